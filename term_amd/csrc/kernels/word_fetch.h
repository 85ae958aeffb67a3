// word_fetch.h -- the bytes of one string value in device memory, a 32-bit word at a time: what the lexer of
// kernels/typeclass.hip and the string leaves of kernels/rowpredicate.hip (string_leaf.h) read values through.
//
// TcWordFetch loads the naturally aligned 32-bit word that holds the byte asked for and keeps it until another word is
// asked for.  Such a word always holds at least one byte of the value, so it lies in the value's allocation
// (allocations start and end on word boundaries); nothing else outside [p, p + len) is read.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace tgx {

typedef const uint32_t __attribute__((address_space(1))) *global_u32_ptr;

struct TcWordFetch {
  uintptr_t p;       // the value's first byte
  uintptr_t at = 1;  // the address of the word in `w` (1: none yet; a word's address is a multiple of 4)
  uint32_t w = 0;
  __device__ __forceinline__ uint8_t operator()(uint64_t i) {
    const uintptr_t a = p + (uintptr_t)i, wa = a & ~(uintptr_t)3;
    if (wa != at) {
      w = *(global_u32_ptr)wa;
      at = wa;
    }
    return (uint8_t)(w >> (8u * (uint32_t)(a & 3)));
  }
  // what string_leaf.h asks of a fetch beside single bytes: how far the value's first byte lies into its word, and the
  // k-th aligned word from the one that holds that byte (the caller asks only for words that hold a byte of the value)
  __device__ __forceinline__ uint32_t misalign() const { return (uint32_t)(p & 3); }
  __device__ __forceinline__ uint32_t word(uint64_t k) {
    const uintptr_t wa = (p & ~(uintptr_t)3) + (uintptr_t)k * 4;
    if (wa != at) {
      w = *(global_u32_ptr)wa;
      at = wa;
    }
    return w;
  }
};

}  // namespace tgx
