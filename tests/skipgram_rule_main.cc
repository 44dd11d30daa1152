// The integer arithmetic of the skip-gram expansion (csrc/bpe_skipgram_rule.h) as a stand-alone host
// program, built by tests/test_skipgram.py with -fsanitize=address,undefined: every pair of every
// text of 0..n_max values for every window 1..w_max against the loop it restates, then texts far
// longer than any test batch at pair numbers around every regime's edge.
//   skipgram_rule_main n_max w_max  ->  "skipgram rule ok <pairs checked>"
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "bpe_skipgram_rule.h"

static int fail(const char *what, long long n, long long w, long long r) {
    std::printf("skipgram rule: %s at n=%lld w=%lld r=%lld\n", what, n, w, r);
    return 1;
}

int main(int argc, char **argv) {
    const long long n_max = argc > 1 ? std::atoll(argv[1]) : 150, w_max = argc > 2 ? std::atoll(argv[2]) : 66;
    long long checked = 0;
    for (long long w = 1; w <= w_max; ++w)
        for (long long n = 0; n <= n_max; ++n) {
            // the loop: for i, for j = i - w .. i + w, skipping j < 0, j == i, j >= n
            std::vector<long long> ti, tj;
            for (long long i = 0; i < n; ++i) {
                if ((long long)ti.size() != sg_before(i, n, w)) return fail("sg_before", n, w, i);
                const size_t at = ti.size();
                for (long long j = i - w; j <= i + w; ++j)
                    if (j >= 0 && j != i && j < n) ti.push_back(i), tj.push_back(j);
                if ((long long)(ti.size() - at) != sg_token_pairs(i, n, w)) return fail("sg_token_pairs", n, w, i);
            }
            if ((long long)ti.size() != sg_text_pairs(n, w)) return fail("sg_text_pairs", n, w, -1);
            if ((long long)ti.size() != sg_before(n, n, w)) return fail("sg_before(n)", n, w, -1);
            for (size_t r = 0; r < ti.size(); ++r) {
                int64_t i = -1, c = -1;
                sg_invert((int64_t)r, n, w, i, c);
                if (i != ti[r] || c < 0 || c >= sg_token_pairs(i, n, w)) return fail("sg_invert", n, w, (long long)r);
                if (sg_context(i, c, w) != tj[r]) return fail("sg_context", n, w, (long long)r);
                ++checked;
            }
        }
    // long texts: pair numbers around the head, the tail and a few tokens of the middle
    const long long longs[] = {(1ll << 20) + 3, (1ll << 24), (1ll << 31) + 5, (1ll << 40) + 1};
    for (long long w = 1; w <= w_max; w += (w < 6 ? 1 : 29))
        for (long long n : longs) {
            const int64_t total = sg_text_pairs(n, w);
            const int64_t spots[] = {0, w * (w + 1), sg_before(n / 2, n, w), sg_before(n - w - 1, n, w), total - w * (w + 1),
                                     total - 1};
            for (int64_t s : spots)
                for (int64_t r = s - 3 * w; r <= s + 3 * w; ++r) {
                    if (r < 0 || r >= total) continue;
                    int64_t i = -1, c = -1;
                    sg_invert(r, n, w, i, c);
                    if (i < 0 || i >= n || sg_before(i, n, w) > r || sg_before(i + 1, n, w) <= r ||
                        c != r - sg_before(i, n, w))
                        return fail("sg_invert (long)", n, w, (long long)r);
                    const int64_t j = sg_context(i, c, w);
                    if (j < 0 || j >= n || j == i || j < i - w || j > i + w) return fail("sg_context (long)", n, w, (long long)r);
                    ++checked;
                }
        }
    std::printf("skipgram rule ok %lld\n", checked);
    return 0;
}
