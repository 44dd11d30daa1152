// bpe_ingest_napi.cc — Node N-API addon of the corpus ingest from text (bpe_set_chars,
// bpe_add_text_batch, include/bpe.h): what js/native.js syncEngineChars and
// BPETokenizer.addToCorpusBatch call.  A module of its own beside bpe_napi.node, over the same
// libbpe.so; it takes the engine handles bpe_napi.node's createEngine makes (napi_util.h
// EngineHolder).  Every function maps 1:1 onto a bpe_* entry point; errors become JS errors carrying
// bpe_last_error().
#define NAPI_VERSION 6
#include <node_api.h>

#include <cstdint>
#include <vector>

#include "bpe.h"
#include "napi_util.h"

namespace {

bpe_ctx *get_ctx(napi_env env, napi_value v) {
    void *p = nullptr;
    if (napi_get_value_external(env, v, &p) != napi_ok || !p) return nullptr;
    return static_cast<EngineHolder *>(p)->c;   // (null after destroyEngine: every call then fails)
}

// a typed array of the given type: its data and length
bool get_typed(napi_env env, napi_value v, napi_typedarray_type want, void **data, size_t *n) {
    napi_typedarray_type t;
    size_t o = 0;
    napi_value ab;
    return napi_get_typedarray_info(env, v, &t, n, data, &ab, &o) == napi_ok && t == want;
}

// setChars(h, Uint32Array code_points, Int32Array ids): replaces the context's char table
// (bpe_set_chars; empty arrays drop it)
napi_value SetChars(napi_env env, napi_callback_info info) {
    napi_value argv[3];
    if (!get_args(env, info, 3, argv)) return throw_arg(env, "setChars(h, Uint32Array, Int32Array)");
    void *cps = nullptr, *ids = nullptr;
    size_t n = 0, m = 0;
    if (!get_typed(env, argv[1], napi_uint32_array, &cps, &n) || !get_typed(env, argv[2], napi_int32_array, &ids, &m) ||
        n != m)
        return throw_arg(env, "setChars expects a Uint32Array of code points and an Int32Array of ids");
    if (bpe_set_chars(get_ctx(env, argv[0]), static_cast<const uint32_t *>(cps), static_cast<const int32_t *>(ids),
                      (int64_t)n) < 0)
        return throw_native(env, "bpe_set_chars");
    return nullptr;
}

// addTextBatch(h, Uint16Array units, Float64Array offsets) -> [Uint32Array newChars, Float64Array
// hist] (bpe_add_text_batch: text k = units[offsets[k] .. offsets[k+1]), every text one sample;
// newChars[i]: the code point of the token numbered (token count before the call) + i; hist[id]:
// this call's occurrences of every id below the token count after it)
napi_value AddTextBatch(napi_env env, napi_callback_info info) {
    napi_value argv[3];
    if (!get_args(env, info, 3, argv)) return throw_arg(env, "addTextBatch(h, Uint16Array, Float64Array)");
    bpe_ctx *ctx = get_ctx(env, argv[0]);
    void *units = nullptr, *offd = nullptr;
    size_t n = 0, n_off = 0;
    if (!get_typed(env, argv[1], napi_uint16_array, &units, &n) ||
        !get_typed(env, argv[2], napi_float64_array, &offd, &n_off) || n_off < 1)
        return throw_arg(env, "addTextBatch expects Uint16Array units and Float64Array offsets");
    std::vector<int64_t> off(n_off);
    const double *d = static_cast<const double *>(offd);
    for (size_t k = 0; k < n_off; ++k) {
        if (!(d[k] >= 0) || d[k] > (double)n) return throw_arg(env, "addTextBatch expects offsets within the units");
        off[k] = (int64_t)d[k];
    }
    std::vector<uint32_t> fresh(BPE_MAX_VOCAB);
    std::vector<int64_t> hist(BPE_MAX_VOCAB);
    int64_t n_new = 0;
    if (bpe_add_text_batch(ctx, static_cast<const uint16_t *>(units), off.data(), (int64_t)n_off - 1, fresh.data(),
                           BPE_MAX_VOCAB, &n_new, hist.data(), BPE_MAX_VOCAB) < 0)
        return throw_native(env, "bpe_add_text_batch");
    int32_t nt = 0;
    if (bpe_num_tokens(ctx, &nt) < 0) return throw_native(env, "bpe_num_tokens");
    napi_value ab_new, ab_hist, a_new, a_hist, out;
    void *pn = nullptr, *ph = nullptr;
    napi_create_arraybuffer(env, (size_t)n_new * 4, &pn, &ab_new);
    napi_create_arraybuffer(env, (size_t)nt * 8, &ph, &ab_hist);
    for (int64_t i = 0; i < n_new; ++i) static_cast<uint32_t *>(pn)[i] = fresh[i];
    for (int32_t i = 0; i < nt; ++i) static_cast<double *>(ph)[i] = (double)hist[i];
    napi_create_typedarray(env, napi_uint32_array, (size_t)n_new, ab_new, 0, &a_new);
    napi_create_typedarray(env, napi_float64_array, (size_t)nt, ab_hist, 0, &a_hist);
    napi_create_array_with_length(env, 2, &out);
    napi_set_element(env, out, 0, a_new);
    napi_set_element(env, out, 1, a_hist);
    return out;
}

napi_value Init(napi_env env, napi_value exports) {
    struct {
        const char *name;
        napi_callback cb;
    } fns[] = {
        {"setChars", SetChars},
        {"addTextBatch", AddTextBatch},
    };
    for (auto &f : fns) {
        napi_value fn;
        napi_create_function(env, f.name, NAPI_AUTO_LENGTH, f.cb, nullptr, &fn);
        napi_set_named_property(env, exports, f.name, fn);
    }
    return exports;
}

}  // namespace

NAPI_MODULE(NODE_GYP_MODULE_NAME, Init)
