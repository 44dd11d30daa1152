// bpe_dropout_rule.h — the integer arithmetic of BPE-dropout (include/bpe.h, "encoding with
// dropout"), apart from the kernel so that a host program can check it on its own
// (tests/dropout_rule_main.cc).  Plain C++; under hipcc every function is __host__ __device__.
// All arithmetic is mod 2^64.
//
// A merge site of a text is named by (i, r): r the merge's rank in the list (below 65536) and i
// the position in the text, before any merge, of the first input token of the site's left token.
// r fixes (a, b), and a starting at i fixes both spans, so (i, r) names one possible merge node of
// the text; it has one coin per (text, sample), whatever order the sites are evaluated in.
#pragma once
#include <cstdint>

#ifdef __HIPCC__
#define DROP_HD __host__ __device__ inline
#else
#define DROP_HD inline
#endif

// the finaliser of splitmix64
DROP_HD uint64_t drop_mix64(uint64_t z) {
    z ^= z >> 30;
    z *= 0xBF58476D1CE4E5B9ull;
    z ^= z >> 27;
    z *= 0x94D049BB133111EBull;
    z ^= z >> 31;
    return z;
}

// the key of sample s (0 <= s < S) of the text with global index t
DROP_HD uint64_t drop_stream(uint64_t seed, uint64_t t, uint64_t s, uint64_t S) {
    return drop_mix64(seed + 0x9E3779B97F4A7C15ull * (t * S + s + 1));
}

// the coin of site (i, r): 32 bits
DROP_HD uint64_t drop_coin(uint64_t stream, uint64_t i, uint32_t r) {
    return drop_mix64(stream ^ ((i << 16) | r)) >> 32;
}

// thr = (uint64_t)(p * 2^32) of the host, 0 <= p <= 1: 0 drops nothing, 2^32 everything
DROP_HD bool drop_dropped(uint64_t stream, uint64_t i, uint32_t r, uint64_t thr) {
    return drop_coin(stream, i, r) < thr;
}

// 0 <= p <= 1 (NaN is neither)
inline bool drop_threshold(double p, uint64_t *thr) {
    if (!(p >= 0.0 && p <= 1.0)) return false;
    *thr = (uint64_t)(p * 4294967296.0);
    return true;
}
