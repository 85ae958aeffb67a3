// typeclass_types.h -- what typeclass_device.cpp hands to kernels/typeclass.hip (TGX_CHECK_TYPE_CLASSES).
//
// A task is one string column.  Per task kTypeClassWords 64-bit global counters at counts[word]: the seven classes in
// the order of kernels/typeclass_lex.h, then the non-NULL rows.
#pragma once
#include <stdint.h>

#include "distinct_types.h"
#include "typeclass_lex.h"

namespace tgx {

constexpr int kTypeClassBlock = 256;
constexpr int kMaxTypeClassPerLaunch = 8;
constexpr int kTcNonNull = kTypeClassCount;
constexpr int kTypeClassWords = kTypeClassCount + 1;

struct TypeClassLaunch {
  Utf8ColDesc cols[kMaxTypeClassPerLaunch];  // (the fingerprint key is not read)
  uint32_t word[kMaxTypeClassPerLaunch];     // first of the task's counters
  unsigned long long *counts;
};

}  // namespace tgx
