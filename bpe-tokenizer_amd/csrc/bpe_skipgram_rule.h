// bpe_skipgram_rule.h — the integer arithmetic of the skip-gram expansion (include/bpe.h, "skip-gram
// pairs"), apart from the kernels so that a host program can check it on its own
// (tests/skipgram_rule_main.cc).  Plain C++; under hipcc every function is __host__ __device__.
//
// One text of n values and window w >= 1.  Token i emits min(i, w) + min(n - 1 - i, w) pairs, its
// contexts j ascending over [i - w, i + w] without i and clipped to [0, n).  The pairs of a text are
// numbered r = 0, 1, ... in emission order; sg_before(i) pairs precede token i's.
#pragma once
#include <cstdint>

#ifdef __HIPCC__
#define SG_HD __host__ __device__ inline
#else
#define SG_HD inline
#endif

// sum of min(t, w) over t in [0, i)
SG_HD int64_t sg_head(int64_t i, int64_t w) {
    return i <= w + 1 ? i * (i - 1) / 2 : w * (w + 1) / 2 + (i - w - 1) * w;
}

// pairs of a text of n values
SG_HD int64_t sg_text_pairs(int64_t n, int64_t w) {
    if (n <= 1) return 0;
    return n <= w + 1 ? n * (n - 1) : w * (2 * n - w - 1);
}

// pairs of token i
SG_HD int64_t sg_token_pairs(int64_t i, int64_t n, int64_t w) {
    const int64_t a = i < w ? i : w, b = n - 1 - i < w ? n - 1 - i : w;
    return a + b;
}

// pairs of the tokens before token i, 0 <= i <= n: the left halves are sg_head(i), the right halves
// mirror the left halves of the last i tokens
SG_HD int64_t sg_before(int64_t i, int64_t n, int64_t w) {
    return sg_head(i, w) + sg_head(n, w) - sg_head(n - i, w);
}

// Pair r of the text, 0 <= r < sg_text_pairs(n, w) (so n >= 2): its token i and its place c among
// that token's pairs.  i is the largest i with sg_before(i) <= r.  No token has more than 2w pairs,
// so i >= r / 2w; all tokens together fall short of 2w each by at most w (w + 1) (the head and the
// tail, which overlap when n < 2w + 1 and then fall short by less), so i <= r / 2w + (w + 1) / 2 + 1.
// The search between the two bounds is exact in integers whatever the regime.
SG_HD void sg_invert(int64_t r, int64_t n, int64_t w, int64_t &i, int64_t &c) {
    int64_t lo = r / (2 * w), hi = lo + (w + 1) / 2 + 1;
    if (hi > n - 1) hi = n - 1;
    if (lo > hi) lo = hi;
    while (lo < hi) {
        const int64_t mid = (lo + hi + 1) >> 1;
        if (sg_before(mid, n, w) <= r) lo = mid;
        else hi = mid - 1;
    }
    i = lo;
    c = r - sg_before(lo, n, w);
}

// the context position of pair c of token i
SG_HD int64_t sg_context(int64_t i, int64_t c, int64_t w) {
    const int64_t j = i - (i < w ? i : w) + c;
    return j + (j >= i ? 1 : 0);
}
