// The dropout rule (csrc/bpe_dropout_rule.h) as a stand-alone host program: prints stream and coin for
// a fixed list of inputs and the number of dropped sites among N coins, for tests/test_encoder_dropout.py
// to compare with its Python restatement.
#include <cinttypes>
#include <cstdio>
#include <initializer_list>

#include "bpe_dropout_rule.h"

int main() {
    const uint64_t seeds[] = {0ull, 1ull, 0xFEDCBA9876543210ull, ~0ull};
    const uint64_t texts[] = {0ull, 1ull, 12345ull, (1ull << 40) + 7};
    for (uint64_t seed : seeds)
        for (uint64_t t : texts)
            for (uint64_t S : {1ull, 3ull})
                for (uint64_t s = 0; s < S; ++s) {
                    const uint64_t st = drop_stream(seed, t, s, S);
                    std::printf("stream %" PRIu64 " %" PRIu64 " %" PRIu64 " %" PRIu64 " %" PRIu64 "\n", seed, t, s, S, st);
                    for (uint64_t i : {0ull, 1ull, 16383ull, 40000ull, (1ull << 47) + 5, (1ull << 50)})
                        for (uint32_t r : {0u, 1u, 999u, 65535u})
                            std::printf("coin %" PRIu64 " %" PRIu64 " %u %" PRIu64 "\n", st, i, r, drop_coin(st, i, r));
                }
    const int N = 100000;
    for (double p : {0.0, 0.1, 0.5, 1.0}) {
        uint64_t thr = 0;
        if (!drop_threshold(p, &thr)) return 1;
        const uint64_t st = drop_stream(0xFEDCBA9876543210ull, 77, 1, 3);
        int dropped = 0;
        for (int i = 0; i < N; ++i) dropped += drop_dropped(st, (uint64_t)i / 8, (uint32_t)(i % 8), thr);
        std::printf("share %.17g %" PRIu64 " %d %d\n", p, thr, N, dropped);
    }
    uint64_t thr = 0;
    if (drop_threshold(-0.5, &thr) || drop_threshold(1.5, &thr) || drop_threshold(__builtin_nan(""), &thr))
        return 2;
    return 0;
}
