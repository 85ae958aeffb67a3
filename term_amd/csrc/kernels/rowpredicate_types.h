// rowpredicate_types.h -- what rowpredicate_device.cpp hands to kernels/rowpredicate.hip (TGX_CHECK_ROW_PREDICATE).
//
// A launch's tasks are descriptors in DEVICE memory (a task is about 2.5 KiB: eight of them do not fit a kernel's
// arguments), one per blockIdx.y; every field is the same for all lanes, so a wave reads it with scalar loads.  The
// host settles per batch, from the type each column arrives in, what a leaf compares (include/tgx.h has the rules): the
// literal as an int64 or as a totalOrder key, and per side whether its bits are doubles.
#pragma once
#include <stdint.h>

#include "distinct_types.h"

namespace tgx {

enum { kRpIsNull = 1, kRpCmpLiteral = 2, kRpCmpColumns = 3, kRpStrEq = 4 };  // TGX_PRED_IS_NULL ..
enum { kRpStrCmp = 6, kRpStrLength = 7, kRpStrLike = 8, kRpStrBlank = 9 };   // TGX_PRED_STR_CMP .. (5 is no kind)
enum { kRpEq = 1, kRpLt = 2, kRpLe = 3, kRpGt = 4, kRpGe = 5 };              // TGX_PRED_EQ ..
enum { kRpPush = 1, kRpAnd = 2, kRpOr = 3, kRpNot = 4 };                     // TGX_PRED_PUSH ..

constexpr int kRowPredBlock = 256;
constexpr int kRowPredMaxLeaves = 32;
constexpr int kRowPredMaxOps = 64;
constexpr int kRowPredMaxLiteralBytes = 256;
constexpr int kRowPredWords = 2;  // satisfied, unknown

struct RowPredLeaf {
  uint8_t kind, op, col, col2;
  uint8_t keyed;             // the sides are compared as totalOrder keys (a float column, or a double literal)
  uint8_t a_float, b_float;  // keyed: col's / col2's bits are doubles already (otherwise int64, converted)
  uint8_t strings;           // CMP_COLUMNS of two string columns: bytes.  STR_LENGTH: the length is in bytes
  uint32_t lit_offset, lit_len;
  // CMP_LITERAL: the int64 literal, or the key of the double literal when keyed.  STR_LENGTH: the length compared
  // with.  STR_LIKE: the pattern's bytes that are not '%' (string_leaf.h's like_min_len)
  int64_t lit;
};

struct RowPredTask {
  TupleDesc d;  // the columns (a numeric one: kind 0 with values / validity / offset) and the batch's rows
  int64_t dict_length[kMaxTupleCols];  // kind 4: an index outside the dictionary is a NULL row
  uint32_t n_leaves, n_ops;
  uint32_t word;       // the task's counters in the state's array
  uint32_t reads;      // bit c: a leaf reads column c's values (an IS_NULL-only column may have none)
  uint32_t keys;       // a leaf is keyed
  uint32_t reserved[3];
  RowPredLeaf leaves[kRowPredMaxLeaves];
  uint16_t program[kRowPredMaxOps];
  uint8_t literals[kRowPredMaxLiteralBytes];
};

}  // namespace tgx
