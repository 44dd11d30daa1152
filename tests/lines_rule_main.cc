// The rule of csrc/bpe_lines.hip.h (ln_classify, ln_next_nw, ln_prev_nw, ln_lf_before, ln_word_bounds,
// ln_text_bounds, ln_length, ln_unit_at) run on the host over a batch of texts as the kernels cut it:
// runs of 8 units into the two bit planes, the tiles' summaries by plain loops, then every plane word
// and every text for the samples' bounds.  tests/test_lines.py builds this with
// -fsanitize=address,undefined and compares what it writes with Node's samples.
//
//   in  (file argv[1]):  int64 n_texts, int64 mis, int64 mode, int64 off[n_texts + 1], uint16 units[off[n_texts]]
//   out (file argv[2]):  int64 n_samples, int64 out_off[n_samples + 1], uint16 units[out_off[n_samples]]
// mis (0..7) shifts the tiles against the batch, as a misaligned unit buffer does; off[0] is 0.
#define BPE_LINES_RULE_ONLY
#include "bpe_lines.hip.h"

#include <cstdio>
#include <vector>

int main(int argc, char **argv) {
    if (argc != 3) return 2;
    FILE *in = std::fopen(argv[1], "rb");
    if (!in) return 2;
    int64_t head[3];
    if (std::fread(head, 8, 3, in) != 3) return 2;
    const int64_t n = head[0];
    const int mis = (int)head[1], mode = (int)head[2];
    std::vector<int64_t> off((size_t)n + 1);
    if (std::fread(off.data(), 8, off.size(), in) != off.size()) return 2;
    const int64_t total = off[(size_t)n];
    std::vector<uint16_t> units((size_t)total);
    if (total && std::fread(units.data(), 2, units.size(), in) != units.size()) return 2;
    std::fclose(in);

    // the batch in slots: slot g holds flat position g - mis (exactly the slots of the batch: a read
    // outside them is a finding)
    std::vector<uint16_t> slots((size_t)(mis + total), 0);
    for (int64_t p = 0; p < total; ++p) slots[(size_t)(mis + p)] = units[(size_t)p];
    const bool lines = mode != BPE_LINES_FILE;
    const int64_t n_tiles = lines ? (total + mis + LN_TILE - 1) / LN_TILE : 0;
    const size_t n_words = (size_t)n_tiles * LN_WORDS;
    std::vector<uint32_t> lf(n_words, 0), nw(n_words, 0), lfpre(n_words, 0);
    std::vector<unsigned long long> nwsum((size_t)n_tiles, 0), tile_base((size_t)n_tiles, 0);
    std::vector<long long> first((size_t)n_tiles, LN_INF), last((size_t)n_tiles, -1);
    for (int64_t g0 = 0; g0 < n_tiles * LN_TILE; g0 += LN_RUN) {   // one lane's run
        uint32_t u[LN_RUN], valid = 0;
        for (int j = 0; j < LN_RUN; ++j) {
            const bool v = g0 + j >= mis && g0 + j < mis + total;
            u[j] = v ? slots[(size_t)(g0 + j)] : 0u;
            valid |= (uint32_t)v << j;
        }
        const LnMasks m = ln_classify(u, valid);
        lf[(size_t)(g0 >> 5)] |= m.lf << (g0 & 31);
        nw[(size_t)(g0 >> 5)] |= m.nw << (g0 & 31);
    }
    int64_t lf_total = 0;
    for (int64_t t = 0; t < n_tiles; ++t) {
        tile_base[(size_t)t] = (unsigned long long)lf_total;
        uint32_t in_tile = 0;
        for (int w = 0; w < LN_WORDS; ++w) {
            const size_t wi = (size_t)(t * LN_WORDS + w);
            lfpre[wi] = in_tile;
            in_tile += (uint32_t)__builtin_popcount(lf[wi]);
            if (!nw[wi]) continue;
            nwsum[(size_t)t] |= 1ull << w;
            if (first[(size_t)t] == LN_INF) first[(size_t)t] = t * LN_TILE + 32 * w + ln_ctz32(nw[wi]);
            last[(size_t)t] = t * LN_TILE + 32 * w + ln_top32(nw[wi]);
        }
        lf_total += in_tile;
    }
    for (int64_t t = n_tiles - 2; t >= 0; --t)
        if (first[(size_t)t + 1] < first[(size_t)t]) first[(size_t)t] = first[(size_t)t + 1];
    for (int64_t t = 1; t < n_tiles; ++t)
        if (last[(size_t)t - 1] > last[(size_t)t]) last[(size_t)t] = last[(size_t)t - 1];

    const int64_t n_samples = lines ? lf_total + n : n;
    std::vector<long long> sb((size_t)n_samples, -7), se((size_t)n_samples, -7);
    if (lines) {
        const LnPlanes P{lf.data(), nw.data(), lfpre.data(), nwsum.data(), tile_base.data(),
                         first.data(), last.data(), n_tiles, lf_total};
        for (size_t wi = 0; wi < n_words; ++wi)
            ln_word_bounds(P, slots.data(), mis, mode, off.data(), n, 0, (int64_t)wi, sb.data(), se.data());
        for (int64_t k = 0; k < n; ++k) ln_text_bounds(P, slots.data(), mis, mode, off.data(), 0, k, sb.data(), se.data());
    } else {
        for (int64_t k = 0; k < n; ++k) sb[(size_t)k] = off[(size_t)k] + mis, se[(size_t)k] = off[(size_t)k + 1] + mis;
    }
    std::vector<int64_t> out_off((size_t)n_samples + 1, 0);
    for (int64_t j = 0; j < n_samples; ++j) {
        if (sb[(size_t)j] == -7 || se[(size_t)j] == -7) return 3;   // (every sample got both its ends)
        out_off[(size_t)j + 1] = out_off[(size_t)j] + ln_length(sb[(size_t)j], se[(size_t)j]);
    }
    std::vector<uint16_t> out((size_t)out_off[(size_t)n_samples]);
    for (int64_t j = 0; j < n_samples; ++j)
        for (int64_t o = out_off[(size_t)j]; o < out_off[(size_t)j + 1]; ++o)
            out[(size_t)o] = (uint16_t)ln_unit_at(slots.data(), mode, o, out_off[(size_t)j], out_off[(size_t)j + 1],
                                                  sb[(size_t)j]);
    FILE *f = std::fopen(argv[2], "wb");
    if (!f) return 2;
    std::fwrite(&n_samples, 8, 1, f);
    std::fwrite(out_off.data(), 8, out_off.size(), f);
    if (!out.empty()) std::fwrite(out.data(), 2, out.size(), f);
    return std::fclose(f) ? 2 : 0;
}
