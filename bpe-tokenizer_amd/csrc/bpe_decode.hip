// bpe_decode.hip — decodeVector / decodeTokens (core.ts:447-471) for many texts at once: batches
// of vector indices or token ids back to UTF-16 code units on the device, behind the
// bpe_decoder_* / bpe_decode_batch entry points of include/bpe.h.
//
// The reference decodes a text by joining its tokens' chars:
//     for (let index of vector) { ... content += token.chars }                    (core.ts:462-468)
// The vocabulary lives on the device as one blob of UTF-16 code units (every token's chars,
// merged tokens materialised: chars[c] = chars[a] + chars[b], core.ts:318,487) and one
// (offset, length) record per token id; the vector index (from_vector_index of compactVectorIndex,
// core.ts:222-241) as one int32 per vector index.  A call is four kernels over tiles of
// BPE_DECODE_TILE values (a value: one vector index or token id of the flat batch):
//   k_dec_texts   one pass over the texts' offsets: their order is checked, and the first text that
//                 starts in each tile is noted (one plain store per tile that has one);
//   k_dec_lens    the values 16 B per lane, value -> id -> length through the tables (L2-resident:
//                 at most 8 B per id), one 64-bit sum per tile (a workgroup takes four tiles, all
//                 loads issued first); a value out of range puts its flat position into a 64-bit
//                 atomicMin (only such lanes do);
//   k_dec_scan    one workgroup: exclusive scan of the tile sums (8192 per round), and the total;
//   k_dec_expand  one workgroup per tile, output-centric: the tile rebuilds its values' exclusive
//                 prefix in LDS; each lane owns runs of 8 consecutive output units cut at 16-B
//                 addresses of the output, finds the token covering its first unit by binary search
//                 in the LDS prefix, walks forward from there and stores 16 B; the workgroup loops
//                 over the tile's output however long it is (a token of thousands of units is
//                 spread over the lanes like any other run).  The same workgroup writes out_off[k]
//                 of the texts that start inside its tile: a strided walk from the tile's first
//                 text, so its cost follows the texts, not the tile size.
// Tiles are cut at 16-B addresses of the value buffer (slot s of tile t holds the flat position
// t * TILE + s - mis, mis = the buffer's misalignment in values), so tokens and texts straddle
// tiles freely and every full load is aligned.  Flat positions, unit counts and tile sums are
// 64-bit.  The kernels talk only across kernel boundaries: k_dec_expand reads the bad-value
// position and the total that the two before it left, and writes nothing when a value was bad, and
// only offsets when the units would not fit.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include "bpe.h"
#include "bpe_multi.h"   // bpe_fail
#include "bpe_utf8_out.hip.h"   // text out as UTF-8: the transcode behind the decode (Utf8OutState)

namespace {

constexpr int TILE = BPE_DECODE_TILE;
constexpr int WG = 256;
constexpr int RUN = 8;   // output units per lane and store (16 B)
constexpr int LENS_TILES = 4;   // tiles per workgroup of k_dec_lens
constexpr int SCAN_EACH = 8;    // tile sums per thread and round of k_dec_scan
static_assert(1024 * SCAN_EACH == BPE_DECODE_SCAN_ROUND, "include/bpe.h");
static_assert(TILE == 4 * WG, "one 16-B load of values per lane");
constexpr unsigned long long NO_BAD = ~0ull;
// status words of a call on the device
constexpr int ST_BAD = 0;      // least flat position of a value out of range (NO_BAD: none)
constexpr int ST_TOTAL = 1;    // units of the whole batch
constexpr int ST_OFF = 2;      // != 0: the offsets decrease somewhere
constexpr int ST_WORDS = 4;

#define DEC_TRY(expr)                                                                      \
    do {                                                                                   \
        hipError_t e_ = (expr);                                                            \
        if (e_ != hipSuccess)                                                              \
            return bpe_fail(e_ == hipErrorOutOfMemory ? BPE_ERR_OOM : BPE_ERR_HIP,         \
                            (std::string("bpe native: ") + #expr + ": " +                   \
                             hipGetErrorString(e_)).c_str());                              \
    } while (0)

struct DecTab {
    const uint2 *rec;        // per token id: (offset into the blob, length), in units
    const int32_t *index;    // vector index -> token id (n_live entries)
    uint32_t n_tokens, n_live;
    int kind;
};

// (offset, length) of one value; bad: the value is out of range
__device__ __forceinline__ uint2 lookup(const DecTab &t, int32_t v, bool &bad) {
    uint32_t id = (uint32_t)v;
    if (t.kind == BPE_DECODE_VECTORS) {
        bad = id >= t.n_live;
        if (bad) return make_uint2(0u, 0u);
        id = (uint32_t)t.index[id];
    } else {
        bad = id >= t.n_tokens;
        if (bad) return make_uint2(0u, 0u);
    }
    return t.rec[id];
}

// This lane's four slots of tile `tile`: flat positions p0 .. p0 + 3; ok[k]: the slot holds a value
// of the batch.  vals_al is the value buffer's 16-B aligned base (the flat position -mis).
__device__ __forceinline__ void load_slots(const int32_t *__restrict__ vals_al, int64_t tile, int mis,
                                           int64_t total, int32_t v[4], bool ok[4], int64_t &p0) {
    const int64_t s = tile * TILE + 4 * (int64_t)threadIdx.x;
    p0 = s - mis;
    if (p0 >= 0 && p0 + 4 <= total) {
        const int4 x = *reinterpret_cast<const int4 *>(vals_al + s);
        v[0] = x.x, v[1] = x.y, v[2] = x.z, v[3] = x.w;
        ok[0] = ok[1] = ok[2] = ok[3] = true;
    } else {
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            ok[k] = p0 + k >= 0 && p0 + k < total;
            v[k] = ok[k] ? vals_al[s + k] : 0;
        }
    }
}

__device__ __forceinline__ unsigned long long wave_incl64(unsigned long long v, int lane) {
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const unsigned long long o = __shfl_up(v, d);
        if (lane >= d) v += o;
    }
    return v;
}

// exclusive prefix and total over the workgroup (one barrier; `s` holds one word per wave)
template <int N>
__device__ __forceinline__ unsigned long long block_scan64(unsigned long long v, unsigned long long *s,
                                                           unsigned long long &total) {
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const unsigned long long incl = wave_incl64(v, lane);
    if (lane == 63) s[w] = incl;
    __syncthreads();
    unsigned long long before = 0, all = 0;
#pragma unroll
    for (int i = 0; i < N / 64; ++i) {
        const unsigned long long x = s[i];
        before += i < w ? x : 0;
        all += x;
    }
    total = all;
    return before + incl - v;
}

// LENS_TILES tiles per workgroup: all their loads are issued before the first is used (a tile is
// 4 KiB of values, too little to hide the two dependent table reads behind)
__global__ void __launch_bounds__(WG)
k_dec_lens(const int32_t *__restrict__ vals_al, int mis, int64_t total, int64_t n_tiles, DecTab t,
           unsigned long long *__restrict__ tile_sum, unsigned long long *__restrict__ st) {
    __shared__ unsigned long long ws[LENS_TILES][WG / 64];
    const int64_t tile0 = (int64_t)blockIdx.x * LENS_TILES;
    int32_t v[LENS_TILES][4];
    bool ok[LENS_TILES][4];
    int64_t p0[LENS_TILES];
#pragma unroll
    for (int g = 0; g < LENS_TILES; ++g) {
        if (tile0 + g < n_tiles) {
            load_slots(vals_al, tile0 + g, mis, total, v[g], ok[g], p0[g]);
        } else {
#pragma unroll
            for (int k = 0; k < 4; ++k) ok[g][k] = false, v[g][k] = 0;
            p0[g] = 0;
        }
    }
    unsigned long long sum[LENS_TILES];
#pragma unroll
    for (int g = 0; g < LENS_TILES; ++g) {
        sum[g] = 0;
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            if (!ok[g][k]) continue;
            bool bad;
            const uint2 r = lookup(t, v[g][k], bad);
            if (bad) atomicMin(&st[ST_BAD], (unsigned long long)(p0[g] + k));
            sum[g] += r.y;
        }
    }
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
#pragma unroll
    for (int g = 0; g < LENS_TILES; ++g) {
        const unsigned long long incl = wave_incl64(sum[g], lane);
        if (lane == 63) ws[g][w] = incl;
    }
    __syncthreads();
    if (threadIdx.x < LENS_TILES && tile0 + threadIdx.x < n_tiles) {
        unsigned long long all = 0;
#pragma unroll
        for (int i = 0; i < WG / 64; ++i) all += ws[threadIdx.x][i];
        tile_sum[tile0 + threadIdx.x] = all;
    }
}

// tile sums -> each tile's base (in place), and the total
__global__ void __launch_bounds__(1024)
k_dec_scan(unsigned long long *__restrict__ tile_sum, int64_t n_tiles, unsigned long long *__restrict__ st) {
    __shared__ unsigned long long ws[16];
    unsigned long long carry = 0;
    for (int64_t b = 0; b < n_tiles; b += 1024 * SCAN_EACH) {
        const int64_t i0 = b + (int64_t)threadIdx.x * SCAN_EACH;
        unsigned long long v[SCAN_EACH], mine = 0;
#pragma unroll
        for (int e = 0; e < SCAN_EACH; ++e) {
            v[e] = i0 + e < n_tiles ? tile_sum[i0 + e] : 0;
            mine += v[e];
        }
        unsigned long long all;
        unsigned long long pre = carry + block_scan64<1024>(mine, ws, all);
#pragma unroll
        for (int e = 0; e < SCAN_EACH; ++e) {
            if (i0 + e < n_tiles) tile_sum[i0 + e] = pre;
            pre += v[e];
        }
        carry += all;
        __syncthreads();   // (ws is reused next round)
    }
    if (threadIdx.x == 0) st[ST_TOTAL] = carry;
}

// One pass over the offsets: off[k + 1] < off[k] anywhere refuses the call (the expand kernel's
// walk relies on the order), and the first text that starts in each tile is noted in tile_first
// (-1 stays where none does).  A text at the very end of the values belongs to the last tile.
__device__ __forceinline__ int64_t tile_of(int64_t p, int mis, int64_t n_tiles) {
    const int64_t t = p < 0 ? 0 : (p + mis) / TILE;
    return t < n_tiles ? t : n_tiles - 1;
}

__global__ void __launch_bounds__(256)
k_dec_texts(const int64_t *__restrict__ off, int64_t n_texts, int64_t base, int mis, int64_t n_tiles,
            long long *__restrict__ tile_first, unsigned long long *__restrict__ st) {
    bool bad = false;
    for (int64_t k = (int64_t)blockIdx.x * 256 + threadIdx.x; k <= n_texts; k += (int64_t)gridDim.x * 256) {
        const int64_t o = off[k];
        if (k < n_texts) bad |= off[k + 1] < o;
        if (n_tiles) {
            const int64_t t = tile_of(o - base, mis, n_tiles);
            if (k == 0 || tile_of(off[k - 1] - base, mis, n_tiles) != t) tile_first[t] = k;
        }
    }
    if (bad) atomicMax(&st[ST_OFF], 1ull);
}

__global__ void __launch_bounds__(WG)
k_dec_expand(const int32_t *__restrict__ vals_al, int mis, int64_t total, DecTab t,
             const uint16_t *__restrict__ blob, const unsigned long long *__restrict__ tile_base,
             const long long *__restrict__ tile_first, const unsigned long long *__restrict__ st,
             const int64_t *__restrict__ off, int64_t n_texts, int64_t base, uint16_t *__restrict__ out,
             int64_t cap, int64_t *__restrict__ out_off) {
    __shared__ unsigned long long s_pre[TILE + 1];   // exclusive prefix of the slots' lengths
    __shared__ uint32_t s_src[TILE];                 // blob offset of each slot's token
    __shared__ unsigned long long ws[WG / 64];
    if (st[ST_BAD] != NO_BAD || st[ST_OFF]) return;   // (uniform: the call is refused)
    const int tid = threadIdx.x;
    const int64_t tile = blockIdx.x;
    const int64_t slot0 = tile * TILE - mis;             // flat position of slot 0
    const int64_t p_lo = slot0 < 0 ? 0 : slot0;   // the tile's flat positions: [p_lo, p_hi)
    const int64_t p_hi = slot0 + TILE < total ? slot0 + TILE : total;

    const long long k0 = tile_first[tile];   // (needed last: the load has the whole kernel to land)
    int32_t v[4];
    bool ok[4];
    int64_t p0;
    load_slots(vals_al, tile, mis, total, v, ok, p0);
    uint2 r[4];
    unsigned long long sum = 0;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        bool bad = false;
        r[k] = ok[k] ? lookup(t, v[k], bad) : make_uint2(0u, 0u);
        sum += r[k].y;
    }
    unsigned long long tsum;
    unsigned long long pre = block_scan64<WG>(sum, ws, tsum);
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        s_pre[4 * tid + k] = pre;
        s_src[4 * tid + k] = r[k].x;
        pre += r[k].y;
    }
    if (tid == 0) s_pre[TILE] = tsum;
    __syncthreads();

    const unsigned long long tb = tile_base[tile];
    if (out && st[ST_TOTAL] <= (unsigned long long)cap && tsum) {
        // runs of RUN units cut at 16-B addresses of `out`: positions shifted by its misalignment
        const unsigned a = (unsigned)((uintptr_t)out >> 1) & (RUN - 1);
        const unsigned long long q_lo = tb + a, q_hi = tb + tsum + a;
        for (unsigned long long c = q_lo / RUN + tid; c * RUN < q_hi; c += WG) {
            const unsigned long long q0 = c * RUN > q_lo ? c * RUN : q_lo;
            const unsigned long long q1 = (c + 1) * RUN < q_hi ? (c + 1) * RUN : q_hi;
            unsigned long long l = q0 - q_lo;   // unit of the tile
            int i = 0, j = TILE;                // the last slot with s_pre[i] <= l (its token is not empty)
            while (j - i > 1) {
                const int m = (i + j) >> 1;
                if (s_pre[m] <= l) i = m; else j = m;
            }
            unsigned long long end = s_pre[i + 1];
            uint32_t src = s_src[i] + (uint32_t)(l - s_pre[i]);
            if (q1 - q0 == RUN) {
                uint32_t w[RUN / 2] = {};
#pragma unroll
                for (int u = 0; u < RUN; ++u) {
                    while (l >= end) {
                        ++i;
                        end = s_pre[i + 1];
                        src = s_src[i];
                    }
                    w[u >> 1] |= (uint32_t)blob[src] << (16 * (u & 1));
                    ++src;
                    ++l;
                }
                *reinterpret_cast<uint4 *>(out + (c * RUN - a)) = make_uint4(w[0], w[1], w[2], w[3]);
            } else {   // (the tile's first and last run: shared with its neighbours)
                for (unsigned long long q = q0; q < q1; ++q) {
                    while (l >= end) {
                        ++i;
                        end = s_pre[i + 1];
                        src = s_src[i];
                    }
                    out[q - a] = blob[src];
                    ++src;
                    ++l;
                }
            }
        }
    }

    // out_off of the texts that start inside the tile (the last tile: also those at the very end)
    const bool last = tile == (int64_t)gridDim.x - 1;
    if (k0 < 0) return;
    for (int64_t k = k0 + tid; k <= n_texts; k += WG) {
        const int64_t p = off[k] - base;
        if (p < p_lo || p > p_hi || (p == p_hi && !last)) break;
        out_off[k] = (int64_t)(tb + s_pre[p - slot0]);
    }
}

}  // namespace

struct bpe_decoder {
    int device = 0;
    hipStream_t stream = nullptr;
    hipEvent_t ev0 = nullptr, ev1 = nullptr;
    // the vocabulary (host copy; the device copy is appended to before a call)
    std::vector<uint16_t> blob;
    std::vector<uint2> rec;
    std::vector<int32_t> index;
    bool has_index = false, index_dirty = false;
    uint16_t *d_blob = nullptr;
    uint2 *d_rec = nullptr;
    int32_t *d_index = nullptr;
    size_t d_blob_cap = 0, d_rec_cap = 0, d_index_cap = 0;
    size_t up_units = 0, up_tokens = 0;   // already on the device
    unsigned long long *d_st = nullptr, *h_st = nullptr;   // status words (h_st pinned)
    unsigned long long *d_tiles = nullptr;   // [tile sums, then bases | first text of each tile]
    size_t d_tiles_cap = 0;
    char *d_buf = nullptr;                // staging of the host form
    size_t d_cap = 0;
    bpe_decoder_stats st{};
    Utf8OutState o8;                      // text out as UTF-8 (bpe_utf8_out.hip.h)
};

namespace {

// grows a device array keeping nothing (the caller uploads again)
template <typename T>
int grow_dev(T **p, size_t *have, size_t want) {
    if (*have >= want) return BPE_OK;
    if (*p) (void)hipFree(*p);
    *p = nullptr;
    *have = 0;
    const size_t n = std::max<size_t>(want, 1) * 3 / 2 + 64;
    DEC_TRY(hipMalloc((void **)p, n * sizeof(T)));
    *have = n;
    return BPE_OK;
}

int upload_vocab(bpe_decoder *D) {
    int rc;
    if (D->up_units == D->blob.size() && D->up_tokens == D->rec.size() && !D->index_dirty) return BPE_OK;
    if (D->d_blob_cap < D->blob.size()) {
        if ((rc = grow_dev(&D->d_blob, &D->d_blob_cap, D->blob.size()))) return rc;
        D->up_units = 0;
    }
    if (D->d_rec_cap < D->rec.size()) {
        if ((rc = grow_dev(&D->d_rec, &D->d_rec_cap, D->rec.size()))) return rc;
        D->up_tokens = 0;
    }
    if (D->up_units < D->blob.size())
        DEC_TRY(hipMemcpyAsync(D->d_blob + D->up_units, D->blob.data() + D->up_units,
                               (D->blob.size() - D->up_units) * 2, hipMemcpyHostToDevice, D->stream));
    if (D->up_tokens < D->rec.size())
        DEC_TRY(hipMemcpyAsync(D->d_rec + D->up_tokens, D->rec.data() + D->up_tokens,
                               (D->rec.size() - D->up_tokens) * sizeof(uint2), hipMemcpyHostToDevice,
                               D->stream));
    if (D->has_index && D->index_dirty) {
        if ((rc = grow_dev(&D->d_index, &D->d_index_cap, D->index.size()))) return rc;
        if (!D->index.empty())
            DEC_TRY(hipMemcpyAsync(D->d_index, D->index.data(), D->index.size() * 4, hipMemcpyHostToDevice,
                                   D->stream));
        D->index_dirty = false;
    }
    // (the host vectors may be appended to right after the call returns: the copies must be done)
    DEC_TRY(hipStreamSynchronize(D->stream));
    D->up_units = D->blob.size();
    D->up_tokens = D->rec.size();
    return BPE_OK;
}

void drop_index(bpe_decoder *D) {
    D->index.clear();
    D->has_index = false;
    D->index_dirty = false;
}

// The pipeline on device buffers.  *wrote_off: out_off holds the call's offsets (also when the
// units did not fit).
int decode_run(bpe_decoder *D, int kind, const int32_t *d_vals, const int64_t *d_off, int64_t n_texts,
               uint16_t *d_out, int64_t cap, int64_t *d_out_off, int64_t *needed, bool *wrote_off) {
    *wrote_off = false;
    if (kind != BPE_DECODE_IDS && kind != BPE_DECODE_VECTORS)
        return bpe_fail(BPE_ERR_ARG, "bpe native: bad decode kind");
    if (n_texts < 0 || cap < 0 || !d_out_off || (n_texts && !d_off) || (cap && !d_out))
        return bpe_fail(BPE_ERR_ARG, "bpe native: bad decode_batch arguments");
    if (kind == BPE_DECODE_VECTORS && !D->has_index)
        return bpe_fail(BPE_ERR_STATE, "bpe native: decode of vectors without a vector index "
                                       "(bpe_decoder_set_vector_index)");
    DEC_TRY(hipSetDevice(D->device));
    int rc;
    if ((rc = upload_vocab(D))) return rc;
    hipStream_t s = D->stream;
    D->st.calls++;
    if (n_texts == 0) {
        DEC_TRY(hipMemsetAsync(d_out_off, 0, 8, s));
        DEC_TRY(hipStreamSynchronize(s));
        *needed = 0;
        *wrote_off = true;
        return BPE_OK;
    }
    int64_t ends[2];
    DEC_TRY(hipMemcpyAsync(&ends[0], d_off, 8, hipMemcpyDeviceToHost, s));
    DEC_TRY(hipMemcpyAsync(&ends[1], d_off + n_texts, 8, hipMemcpyDeviceToHost, s));
    DEC_TRY(hipStreamSynchronize(s));
    const int64_t base = ends[0], total = ends[1] - ends[0];
    if (base < 0) return bpe_fail(BPE_ERR_ARG, "bpe native: negative text offset");
    if (total < 0) return bpe_fail(BPE_ERR_ARG, "bpe native: text offsets must not decrease");
    if (total && !d_vals) return bpe_fail(BPE_ERR_ARG, "bpe native: null value buffer");
    const int mis = total ? (int)(((uintptr_t)(d_vals + base) >> 2) & 3) : 0;
    const int64_t n_tiles = (total + mis + TILE - 1) / TILE;
    if (n_tiles > 0x7FFFFFFF) return bpe_fail(BPE_ERR_ARG, "bpe native: decode batch too large");
    if ((rc = grow_dev(&D->d_tiles, &D->d_tiles_cap, 2 * (size_t)n_tiles))) return rc;
    long long *tile_first = reinterpret_cast<long long *>(D->d_tiles + n_tiles);
    DEC_TRY(hipMemsetAsync(D->d_st, 0xFF, 8, s));
    DEC_TRY(hipMemsetAsync(D->d_st + 1, 0, (ST_WORDS - 1) * 8, s));
    const DecTab t{D->d_rec, D->d_index, (uint32_t)D->rec.size(),
                   (uint32_t)(kind == BPE_DECODE_VECTORS ? D->index.size() : 0), kind};
    const int32_t *vals_al = total ? d_vals + base - mis : nullptr;
    DEC_TRY(hipEventRecord(D->ev0, s));
    if (n_tiles) DEC_TRY(hipMemsetAsync(tile_first, 0xFF, (size_t)n_tiles * 8, s));
    k_dec_texts<<<(unsigned)std::min<int64_t>((n_texts + 256) / 256, 2048), 256, 0, s>>>(
        d_off, n_texts, base, mis, n_tiles, tile_first, D->d_st);
    if (n_tiles) {
        k_dec_lens<<<(unsigned)((n_tiles + LENS_TILES - 1) / LENS_TILES), WG, 0, s>>>(vals_al, mis, total, n_tiles,
                                                                                     t, D->d_tiles, D->d_st);
        k_dec_scan<<<1, 1024, 0, s>>>(D->d_tiles, n_tiles, D->d_st);
        k_dec_expand<<<(unsigned)n_tiles, WG, 0, s>>>(vals_al, mis, total, t, D->d_blob, D->d_tiles, tile_first,
                                                      D->d_st, d_off, n_texts, base, d_out, cap, d_out_off);
    }
    DEC_TRY(hipGetLastError());
    DEC_TRY(hipEventRecord(D->ev1, s));
    DEC_TRY(hipMemcpyAsync(D->h_st, D->d_st, ST_WORDS * 8, hipMemcpyDeviceToHost, s));
    DEC_TRY(hipStreamSynchronize(s));
    float ms = 0;
    DEC_TRY(hipEventElapsedTime(&ms, D->ev0, D->ev1));
    D->st.kernel_ms += ms;
    if (D->h_st[ST_OFF]) return bpe_fail(BPE_ERR_ARG, "bpe native: text offsets must not decrease");
    if (!n_tiles) {   // (every text is empty)
        DEC_TRY(hipMemsetAsync(d_out_off, 0, (size_t)(n_texts + 1) * 8, s));
        DEC_TRY(hipStreamSynchronize(s));
    }
    if (D->h_st[ST_BAD] != NO_BAD) {
        // the first offending value in flat order: the one the reference's loop throws on
        const int64_t p = (int64_t)D->h_st[ST_BAD];
        int32_t v = 0;
        std::vector<int64_t> off((size_t)n_texts + 1);
        DEC_TRY(hipMemcpyAsync(&v, d_vals + base + p, 4, hipMemcpyDeviceToHost, s));
        DEC_TRY(hipMemcpyAsync(off.data(), d_off, off.size() * 8, hipMemcpyDeviceToHost, s));
        DEC_TRY(hipStreamSynchronize(s));
        const int64_t k = (std::upper_bound(off.begin(), off.end(), base + p) - off.begin()) - 1;
        char msg[160];
        std::snprintf(msg, sizeof msg, "unknown %s index: %d (text %lld, position %lld)",
                      kind == BPE_DECODE_VECTORS ? "vector" : "token", v, (long long)k,
                      (long long)(base + p - off[(size_t)k]));
        return bpe_fail(BPE_ERR_VOCAB, msg);
    }
    *needed = (int64_t)D->h_st[ST_TOTAL];
    *wrote_off = true;
    D->st.texts += n_texts;
    D->st.values_in += total;
    if (*needed > cap) {
        char msg[128];
        std::snprintf(msg, sizeof msg, "bpe native: decode needs %lld units, the buffer holds %lld",
                      (long long)*needed, (long long)cap);
        return bpe_fail(BPE_ERR_ARG, msg);
    }
    D->st.units_out += *needed;
    return BPE_OK;
}

size_t align16(size_t x) { return (x + 15) & ~(size_t)15; }

// ---- text out as UTF-8 (include/bpe.h; the kernels and the transcode: bpe_utf8_out.hip.h) ---------

// The end of a transcode call: the capacity answer and the counters.  *needed: the bytes, once the
// offsets are written.
int utf8_out_result(bpe_decoder *D, const Utf8OutCall &J, int rc, int64_t *needed) {
    if (rc) return rc;
    *needed = J.bytes;
    if (!J.fits) return u16_cap_error(J);
    u16_commit(D->o8, J);
    return BPE_OK;
}

// ... of a host form: the offsets and, when they fit, the bytes come back from the scratch.
int utf8_out_to_host(bpe_decoder *D, const Utf8OutCall &J, int rc, uint8_t *bytes_out, int64_t *out_off) {
    int64_t needed = -1;
    rc = utf8_out_result(D, J, rc, &needed);
    if (needed < 0) return rc;
    DEC_TRY(hipMemcpyAsync(out_off, J.d_boff, (size_t)(J.n_texts + 1) * 8, hipMemcpyDeviceToHost, D->stream));
    if (rc == BPE_OK && needed)
        DEC_TRY(hipMemcpyAsync(bytes_out, J.d_bytes, (size_t)needed, hipMemcpyDeviceToHost, D->stream));
    DEC_TRY(hipStreamSynchronize(D->stream));
    return rc;   // (with the capacity message, when it did not fit)
}

// bpe_decode_batch_device into the decoder's scratch (a sizing pass, then the units), and the
// transcode of those units.  J holds the byte outputs and their capacity.  The decoder's own errors
// come back as they are, with J untouched and *transcoded false.
// bpe_decoder_stats sees one decode per call: the sizing pass's counters are dropped when the units
// pass follows (its kernel time stays); when nothing follows (a decoder error, or every text empty)
// the first pass is the call.  They count the decode even when the bytes then miss their capacity:
// what became of the bytes is in bpe_utf8_stats.
int decode_utf8_run(bpe_decoder *D, int kind, const int32_t *d_vals, const int64_t *d_off, int64_t n_texts,
                    Utf8OutCall &J, bool *transcoded) {
    Utf8OutState &U = D->o8;
    *transcoded = false;
    DEC_TRY(hipSetDevice(D->device));
    const size_t b_off = align16((size_t)(n_texts + 1) * 8);
    int rc;
    if ((rc = u16_grow(D->stream, &U.d_dec, &U.d_dec_cap, b_off))) return rc;
    const bpe_decoder_stats keep = D->st;
    int64_t units = 0;
    bool wrote = false;
    rc = decode_run(D, kind, d_vals, d_off, n_texts, nullptr, 0, reinterpret_cast<int64_t *>(U.d_dec), &units, &wrote);
    if (rc && !(rc == BPE_ERR_ARG && wrote && units > 0)) return rc;
    if (units > 0) {
        const double ms = D->st.kernel_ms;
        D->st = keep;   // (one call, asked twice)
        D->st.kernel_ms = ms;
        if ((rc = u16_grow(D->stream, &U.d_dec, &U.d_dec_cap, b_off + (size_t)units * 2))) return rc;
        rc = decode_run(D, kind, d_vals, d_off, n_texts, reinterpret_cast<uint16_t *>(U.d_dec + b_off), units,
                        reinterpret_cast<int64_t *>(U.d_dec), &units, &wrote);
        if (rc) return rc;
    }
    J.units = reinterpret_cast<const uint16_t *>(U.d_dec + b_off);
    J.off = reinterpret_cast<const int64_t *>(U.d_dec);
    J.n_texts = n_texts;
    J.dev = true;
    *transcoded = true;
    return u16_transcode(U, D->stream, J);
}

}  // namespace

int decoder_device(bpe_decoder *D, int *device) {
    if (!D || !device) return bpe_fail(BPE_ERR_ARG, "bpe native: null decoder");
    *device = D->device;
    return BPE_OK;
}

extern "C" {

int bpe_decoder_create(bpe_decoder **out, int device) {
    if (!out) return bpe_fail(BPE_ERR_ARG, "bpe native: null argument");
    *out = nullptr;
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess || n == 0)
        return bpe_fail(BPE_ERR_HIP, "bpe native: no HIP device available (MI355X required)");
    if (device < 0 || device >= n) return bpe_fail(BPE_ERR_ARG, "bpe native: bad device index");
    bpe_decoder *D = new bpe_decoder();
    D->device = device;
    auto bail = [&](int rc) {
        bpe_decoder_destroy(D);
        return rc;
    };
    if (hipSetDevice(device) != hipSuccess ||
        hipStreamCreateWithFlags(&D->stream, hipStreamNonBlocking) != hipSuccess ||
        hipEventCreate(&D->ev0) != hipSuccess || hipEventCreate(&D->ev1) != hipSuccess)
        return bail(bpe_fail(BPE_ERR_HIP, "bpe native: decoder stream/events"));
    if (hipMalloc((void **)&D->d_st, ST_WORDS * 8) != hipSuccess ||
        hipHostMalloc((void **)&D->h_st, ST_WORDS * 8, hipHostMallocDefault) != hipSuccess)
        return bail(bpe_fail(BPE_ERR_OOM, "bpe native: decoder status words"));
    *out = D;
    return BPE_OK;
}

int bpe_decoder_destroy(bpe_decoder *D) {
    if (!D) return BPE_OK;
    (void)hipSetDevice(D->device);
    if (D->stream) (void)hipStreamSynchronize(D->stream);
    if (D->d_blob) (void)hipFree(D->d_blob);
    if (D->d_rec) (void)hipFree(D->d_rec);
    if (D->d_index) (void)hipFree(D->d_index);
    if (D->d_st) (void)hipFree(D->d_st);
    if (D->h_st) (void)hipHostFree(D->h_st);
    if (D->d_tiles) (void)hipFree(D->d_tiles);
    if (D->d_buf) (void)hipFree(D->d_buf);
    u16_free(D->o8);
    if (D->ev0) (void)hipEventDestroy(D->ev0);
    if (D->ev1) (void)hipEventDestroy(D->ev1);
    if (D->stream) (void)hipStreamDestroy(D->stream);
    delete D;
    return BPE_OK;
}

int bpe_decoder_clear(bpe_decoder *D) {
    if (!D) return bpe_fail(BPE_ERR_ARG, "bpe native: null decoder");
    D->blob.clear();
    D->rec.clear();
    D->up_units = D->up_tokens = 0;
    drop_index(D);
    return BPE_OK;
}

int bpe_decoder_add_tokens(bpe_decoder *D, const uint16_t *units, const int64_t *off, int64_t n) {
    if (!D || n < 0 || (n && !off)) return bpe_fail(BPE_ERR_ARG, "bpe native: bad add_tokens arguments");
    if (n == 0) return BPE_OK;
    if (off[0] < 0) return bpe_fail(BPE_ERR_ARG, "bpe native: negative token offset");
    for (int64_t k = 0; k < n; ++k)
        if (off[k + 1] < off[k]) return bpe_fail(BPE_ERR_ARG, "bpe native: token offsets must not decrease");
    const int64_t add = off[n] - off[0];
    if (add && !units) return bpe_fail(BPE_ERR_ARG, "bpe native: null unit buffer");
    if ((int64_t)D->rec.size() + n > BPE_MAX_VOCAB)
        return bpe_fail(BPE_ERR_VOCAB, "bpe native: token id out of range (BPE_MAX_VOCAB)");
    if ((uint64_t)D->blob.size() + (uint64_t)add > 0xFFFFFFFFull)
        return bpe_fail(BPE_ERR_VOCAB, "bpe native: the vocabulary's chars pass 2^32 UTF-16 units");
    const uint32_t at = (uint32_t)D->blob.size();
    if (add) D->blob.insert(D->blob.end(), units + off[0], units + off[n]);
    for (int64_t k = 0; k < n; ++k)
        D->rec.push_back(make_uint2(at + (uint32_t)(off[k] - off[0]), (uint32_t)(off[k + 1] - off[k])));
    drop_index(D);
    return BPE_OK;
}

int bpe_decoder_add_merges(bpe_decoder *D, const int32_t *abc, int64_t n) {
    if (!D || n < 0 || (n && !abc)) return bpe_fail(BPE_ERR_ARG, "bpe native: bad add_merges arguments");
    if (n == 0) return BPE_OK;
    // checked first: a failed call adds nothing
    const int64_t count = (int64_t)D->rec.size();
    std::vector<uint32_t> len((size_t)n);
    uint64_t units = D->blob.size();
    for (int64_t i = 0; i < n; ++i) {
        const int64_t a = abc[3 * i], b = abc[3 * i + 1], c = abc[3 * i + 2], now = count + i;
        if (c != now) {
            char msg[128];
            std::snprintf(msg, sizeof msg, "bpe native: merge %lld makes token %lld, the next id is %lld",
                          (long long)i, (long long)c, (long long)now);
            return bpe_fail(BPE_ERR_ARG, msg);
        }
        if (a < 0 || b < 0 || a >= now || b >= now)
            return bpe_fail(BPE_ERR_VOCAB, "bpe native: merge input is not a known token");
        if (now >= BPE_MAX_VOCAB)
            return bpe_fail(BPE_ERR_VOCAB, "bpe native: token id out of range (BPE_MAX_VOCAB)");
        const uint64_t la = a < count ? D->rec[(size_t)a].y : len[(size_t)(a - count)];
        const uint64_t lb = b < count ? D->rec[(size_t)b].y : len[(size_t)(b - count)];
        units += la + lb;
        if (units > 0xFFFFFFFFull)
            return bpe_fail(BPE_ERR_VOCAB, "bpe native: the vocabulary's chars pass 2^32 UTF-16 units");
        len[(size_t)i] = (uint32_t)(la + lb);
    }
    D->blob.reserve((size_t)units);
    for (int64_t i = 0; i < n; ++i) {
        const uint2 ra = D->rec[(size_t)abc[3 * i]], rb = D->rec[(size_t)abc[3 * i + 1]];
        const uint32_t at = (uint32_t)D->blob.size();
        D->blob.resize((size_t)at + ra.y + rb.y);
        uint16_t *p = D->blob.data();
        std::memcpy(p + at, p + ra.x, (size_t)ra.y * 2);
        std::memcpy(p + at + ra.y, p + rb.x, (size_t)rb.y * 2);
        D->rec.push_back(make_uint2(at, ra.y + rb.y));
    }
    drop_index(D);
    return BPE_OK;
}

int bpe_decoder_num_tokens(bpe_decoder *D, int32_t *n_tokens, int64_t *n_units) {
    if (!D) return bpe_fail(BPE_ERR_ARG, "bpe native: null decoder");
    if (n_tokens) *n_tokens = (int32_t)D->rec.size();
    if (n_units) *n_units = (int64_t)D->blob.size();
    return BPE_OK;
}

int bpe_decoder_set_vector_index(bpe_decoder *D, const int32_t *from_vector_index, int32_t n) {
    if (!D || n < 0 || (n && !from_vector_index))
        return bpe_fail(BPE_ERR_ARG, "bpe native: bad set_vector_index arguments");
    if (n == 0 && !from_vector_index) {
        drop_index(D);
        return BPE_OK;
    }
    for (int32_t i = 0; i < n; ++i)
        if (from_vector_index[i] < 0 || (size_t)from_vector_index[i] >= D->rec.size())
            return bpe_fail(BPE_ERR_VOCAB, "bpe native: vector index names an unknown token");
    D->index.assign(from_vector_index, from_vector_index + n);
    D->has_index = true;
    D->index_dirty = true;
    return BPE_OK;
}

int bpe_decode_batch_device(bpe_decoder *D, int kind, const int32_t *d_vals, const int64_t *d_off,
                            int64_t n_texts, uint16_t *d_units_out, int64_t units_cap,
                            int64_t *d_out_off, int64_t *needed) {
    if (!D || !needed) return bpe_fail(BPE_ERR_ARG, "bpe native: null argument");
    bool wrote = false;
    return decode_run(D, kind, d_vals, d_off, n_texts, d_units_out, units_cap, d_out_off, needed, &wrote);
}

int bpe_decode_batch(bpe_decoder *D, int kind, const int32_t *vals, const int64_t *off, int64_t n_texts,
                     uint16_t *units_out, int64_t units_cap, int64_t *out_off) {
    if (!D || n_texts < 0 || units_cap < 0 || !out_off || (n_texts && !off) || (units_cap && !units_out))
        return bpe_fail(BPE_ERR_ARG, "bpe native: bad decode_batch arguments");
    if (n_texts && off[0] < 0) return bpe_fail(BPE_ERR_ARG, "bpe native: negative text offset");
    for (int64_t k = 0; k < n_texts; ++k)
        if (off[k + 1] < off[k]) return bpe_fail(BPE_ERR_ARG, "bpe native: text offsets must not decrease");
    const int64_t base = n_texts ? off[0] : 0, total = n_texts ? off[n_texts] - base : 0;
    if (total && !vals) return bpe_fail(BPE_ERR_ARG, "bpe native: null value buffer");
    DEC_TRY(hipSetDevice(D->device));
    // device staging: [vals | off (n+1) | out_off (n+1) | units]
    const size_t b_vals = align16((size_t)total * 4), b_off = align16((size_t)(n_texts + 1) * 8);
    const size_t bytes = b_vals + 2 * b_off + align16((size_t)units_cap * 2);
    int rc;
    if ((rc = grow_dev(&D->d_buf, &D->d_cap, bytes))) return rc;
    int32_t *d_vals = reinterpret_cast<int32_t *>(D->d_buf);
    int64_t *d_off = reinterpret_cast<int64_t *>(D->d_buf + b_vals);
    int64_t *d_ooff = reinterpret_cast<int64_t *>(D->d_buf + b_vals + b_off);
    uint16_t *d_units = reinterpret_cast<uint16_t *>(D->d_buf + b_vals + 2 * b_off);
    std::vector<int64_t> rel((size_t)n_texts + 1, 0);
    for (int64_t k = 0; k <= n_texts && n_texts; ++k) rel[(size_t)k] = off[k] - base;
    if (total) DEC_TRY(hipMemcpyAsync(d_vals, vals + base, (size_t)total * 4, hipMemcpyHostToDevice, D->stream));
    DEC_TRY(hipMemcpyAsync(d_off, rel.data(), rel.size() * 8, hipMemcpyHostToDevice, D->stream));
    DEC_TRY(hipStreamSynchronize(D->stream));   // (rel goes away with this frame)
    int64_t needed = 0;
    bool wrote = false;
    rc = decode_run(D, kind, d_vals, d_off, n_texts, units_cap ? d_units : nullptr, units_cap, d_ooff,
                    &needed, &wrote);
    if (wrote) {
        DEC_TRY(hipMemcpyAsync(out_off, d_ooff, (size_t)(n_texts + 1) * 8, hipMemcpyDeviceToHost, D->stream));
        if (rc == BPE_OK && needed)
            DEC_TRY(hipMemcpyAsync(units_out, d_units, (size_t)needed * 2, hipMemcpyDeviceToHost, D->stream));
        DEC_TRY(hipStreamSynchronize(D->stream));
    }
    return rc;
}

int bpe_decoder_get_stats(bpe_decoder *D, bpe_decoder_stats *out) {
    if (!D || !out) return bpe_fail(BPE_ERR_ARG, "bpe native: null argument");
    *out = D->st;
    return BPE_OK;
}

int bpe_decoder_reset_stats(bpe_decoder *D) {
    if (!D) return bpe_fail(BPE_ERR_ARG, "bpe native: null argument");
    D->st = bpe_decoder_stats{};
    return BPE_OK;
}

int bpe_decoder_utf16_to_utf8_device(bpe_decoder *D, const uint16_t *d_units, const int64_t *d_off, int64_t n_texts,
                                     uint8_t *d_bytes_out, int64_t bytes_cap, int64_t *d_out_off, int64_t *needed) {
    if (!D || !needed || n_texts < 0 || bytes_cap < 0 || !d_out_off || (n_texts && !d_off) ||
        (bytes_cap && !d_bytes_out))
        return bpe_fail(BPE_ERR_ARG, "bpe native: bad utf16_to_utf8 arguments");
    DEC_TRY(hipSetDevice(D->device));
    D->o8.st.calls++;
    Utf8OutCall J;
    J.units = d_units, J.off = d_off, J.n_texts = n_texts, J.dev = true;
    J.d_bytes = d_bytes_out, J.d_boff = d_out_off, J.cap = bytes_cap;
    return utf8_out_result(D, J, u16_transcode(D->o8, D->stream, J), needed);
}

int bpe_decoder_utf16_to_utf8(bpe_decoder *D, const uint16_t *units, const int64_t *off, int64_t n_texts,
                              uint8_t *bytes_out, int64_t bytes_cap, int64_t *out_off) {
    if (!D || n_texts < 0 || bytes_cap < 0 || !out_off || (n_texts && !off) || (bytes_cap && !bytes_out))
        return bpe_fail(BPE_ERR_ARG, "bpe native: bad utf16_to_utf8 arguments");
    DEC_TRY(hipSetDevice(D->device));
    D->o8.st.calls++;
    Utf8OutCall J;
    J.units = units, J.off = off, J.n_texts = n_texts, J.cap = bytes_cap;
    return utf8_out_to_host(D, J, u16_transcode(D->o8, D->stream, J), bytes_out, out_off);
}

int bpe_decode_utf8_batch_device(bpe_decoder *D, int kind, const int32_t *d_vals, const int64_t *d_off,
                                 int64_t n_texts, uint8_t *d_bytes_out, int64_t bytes_cap, int64_t *d_out_off,
                                 int64_t *needed) {
    if (!D || !needed || n_texts < 0 || bytes_cap < 0 || !d_out_off || (n_texts && !d_off) ||
        (bytes_cap && !d_bytes_out))
        return bpe_fail(BPE_ERR_ARG, "bpe native: bad decode_utf8_batch arguments");
    D->o8.st.calls++;
    Utf8OutCall J;
    J.d_bytes = d_bytes_out, J.d_boff = d_out_off, J.cap = bytes_cap;
    bool transcoded = false;
    const int rc = decode_utf8_run(D, kind, d_vals, d_off, n_texts, J, &transcoded);
    return transcoded ? utf8_out_result(D, J, rc, needed) : rc;
}

int bpe_decode_utf8_batch(bpe_decoder *D, int kind, const int32_t *vals, const int64_t *off, int64_t n_texts,
                          uint8_t *bytes_out, int64_t bytes_cap, int64_t *out_off) {
    if (!D || n_texts < 0 || bytes_cap < 0 || !out_off || (n_texts && !off) || (bytes_cap && !bytes_out))
        return bpe_fail(BPE_ERR_ARG, "bpe native: bad decode_utf8_batch arguments");
    if (n_texts && off[0] < 0) return bpe_fail(BPE_ERR_ARG, "bpe native: negative text offset");
    for (int64_t k = 0; k < n_texts; ++k)
        if (off[k + 1] < off[k]) return bpe_fail(BPE_ERR_ARG, "bpe native: text offsets must not decrease");
    const int64_t base = n_texts ? off[0] : 0, total = n_texts ? off[n_texts] - base : 0;
    if (total && !vals) return bpe_fail(BPE_ERR_ARG, "bpe native: null value buffer");
    DEC_TRY(hipSetDevice(D->device));
    D->o8.st.calls++;
    // device staging: [vals | off (n+1)]
    const size_t b_vals = align16((size_t)total * 4), b_off = align16((size_t)(n_texts + 1) * 8);
    int rc;
    if ((rc = grow_dev(&D->d_buf, &D->d_cap, b_vals + b_off))) return rc;
    int32_t *d_vals = reinterpret_cast<int32_t *>(D->d_buf);
    int64_t *d_off = reinterpret_cast<int64_t *>(D->d_buf + b_vals);
    std::vector<int64_t> rel((size_t)n_texts + 1, 0);
    for (int64_t k = 0; k <= n_texts && n_texts; ++k) rel[(size_t)k] = off[k] - base;
    if (total) DEC_TRY(hipMemcpyAsync(d_vals, vals + base, (size_t)total * 4, hipMemcpyHostToDevice, D->stream));
    DEC_TRY(hipMemcpyAsync(d_off, rel.data(), rel.size() * 8, hipMemcpyHostToDevice, D->stream));
    DEC_TRY(hipStreamSynchronize(D->stream));   // (rel goes away with this frame)
    Utf8OutCall J;
    J.cap = bytes_cap;
    bool transcoded = false;
    rc = decode_utf8_run(D, kind, d_vals, d_off, n_texts, J, &transcoded);
    return transcoded ? utf8_out_to_host(D, J, rc, bytes_out, out_off) : rc;
}

int bpe_decoder_get_utf8_stats(bpe_decoder *D, bpe_utf8_stats *out) {
    if (!D || !out) return bpe_fail(BPE_ERR_ARG, "bpe native: null argument");
    *out = D->o8.st;
    return BPE_OK;
}

int bpe_decoder_reset_utf8_stats(bpe_decoder *D) {
    if (!D) return bpe_fail(BPE_ERR_ARG, "bpe native: null argument");
    D->o8.st = bpe_utf8_stats{};
    return BPE_OK;
}

}  // extern "C"
