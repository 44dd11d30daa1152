// The per-lane rule of csrc/bpe_utf8_out.hip.h (u16_classify, u16_bytes_in, u16_bytes_at) run on the
// host over a batch of texts, lane by lane as the kernels cut it: runs of 8 units with one halo unit
// on each side and the texts' starts as bits.  tests/test_utf8_out.py builds this with
// -fsanitize=address,undefined and compares what it writes with Node's bytes.
//
//   in  (file argv[1]):  int64 n_texts, int64 mis, int64 off[n_texts + 1], uint16 units[off[n_texts]]
//   out (file argv[2]):  int64 replaced, int64 out_off[n_texts + 1], uint8 bytes[out_off[n_texts]]
// mis (0..7) shifts the runs against the batch, as a misaligned unit buffer does.
#define BPE_UTF8_OUT_CLASSIFY_ONLY
#include "bpe_utf8_out.hip.h"

#include <cstdio>
#include <vector>

int main(int argc, char **argv) {
    if (argc != 3) return 2;
    FILE *in = std::fopen(argv[1], "rb");
    if (!in) return 2;
    int64_t head[2];
    if (std::fread(head, 8, 2, in) != 2) return 2;
    const int64_t n = head[0], mis = head[1];
    std::vector<int64_t> off((size_t)n + 1);
    if (std::fread(off.data(), 8, off.size(), in) != off.size()) return 2;
    const int64_t total = off[(size_t)n];
    std::vector<uint16_t> units((size_t)total);
    if (total && std::fread(units.data(), 2, units.size(), in) != units.size()) return 2;
    std::fclose(in);

    std::vector<char> starts((size_t)total + 1, 0);   // a text starts at this flat position
    for (int64_t k = 0; k < n; ++k)
        if (off[(size_t)k] < total) starts[(size_t)off[(size_t)k]] = 1;
    std::vector<int64_t> before((size_t)total + 1, 0);   // bytes before each flat position
    std::vector<uint8_t> bytes;
    int64_t replaced = 0;
    auto at = [&](int64_t p) -> uint32_t { return p >= 0 && p < total ? units[(size_t)p] : 0u; };
    for (int64_t p0 = -mis; p0 < total; p0 += U16_RUN) {
        uint32_t u[U16_N], f = 0, valid = 0;
        for (int s = 0; s < U16_N; ++s) u[s] = at(p0 - 1 + s);
        for (int j = 0; j <= U16_RUN; ++j)
            if (p0 + j >= 0 && p0 + j < total && starts[(size_t)(p0 + j)]) f |= 1u << (j + 1);
        for (int j = 0; j < U16_RUN; ++j)
            if (p0 + j >= 0 && p0 + j < total) valid |= 1u << j;
        const U16Masks m = u16_classify(u, f, valid);
        const size_t run0 = bytes.size();
        for (int j = 0; j < U16_RUN; ++j) {
            if (p0 + j < 0 || p0 + j >= total) continue;
            before[(size_t)(p0 + j)] = (int64_t)run0 + u16_bytes_in(m, (1u << j) - 1u);
            if (!((m.start >> j) & 1)) continue;
            uint32_t b[4];
            const int k = u16_bytes_at(u, m, j, b);
            for (int i = 0; i < k; ++i) bytes.push_back((uint8_t)b[i]);
        }
        if ((int64_t)(bytes.size() - run0) != u16_bytes_in(m, 0xFFu)) return 3;   // (count and map agree)
        replaced += __builtin_popcount(m.repl);
    }
    before[(size_t)total] = (int64_t)bytes.size();
    std::vector<int64_t> out_off((size_t)n + 1);
    for (int64_t k = 0; k <= n; ++k) out_off[(size_t)k] = before[(size_t)off[(size_t)k]];
    FILE *out = std::fopen(argv[2], "wb");
    if (!out) return 2;
    std::fwrite(&replaced, 8, 1, out);
    std::fwrite(out_off.data(), 8, out_off.size(), out);
    if (!bytes.empty()) std::fwrite(bytes.data(), 1, bytes.size(), out);
    return std::fclose(out) ? 2 : 0;
}
