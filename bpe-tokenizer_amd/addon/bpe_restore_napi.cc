// bpe_restore_napi.cc — Node N-API addon of the corpus from encoded samples and the restore
// (bpe_add_sample_batch, bpe_restore_text_batch, include/bpe.h): what BPETokenizer.restoreToCorpusBatch
// calls.  A module of its own beside bpe_napi.node, over the same libbpe.so; it takes the engine
// handles bpe_napi.node's createEngine makes and the text encoder handles bpe_text_napi.node's
// createTextEncoder makes (napi_util.h EngineHolder, TextEncoderHolder).  Every function maps 1:1
// onto a bpe_* entry point; errors become JS errors carrying bpe_last_error().
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

bpe_encoder *get_encoder(napi_env env, napi_value v) {
    void *p = nullptr;
    if (napi_get_value_external(env, v, &p) != napi_ok || !p) return nullptr;
    return static_cast<TextEncoderHolder *>(p)->e;   // (null after destroyTextEncoder)
}

// a typed array of the given type: its data and length
bool get_typed(napi_env env, napi_value v, napi_typedarray_type want, void **data, size_t *n) {
    napi_typedarray_type t;
    size_t o = 0;
    napi_value ab;
    return napi_get_typedarray_info(env, v, &t, n, data, &ab, &o) == napi_ok && t == want;
}

// Float64Array offsets within [0, n] -> int64
bool get_offsets(const void *offd, size_t n_off, size_t n, std::vector<int64_t> &off) {
    off.resize(n_off);
    const double *d = static_cast<const double *>(offd);
    for (size_t k = 0; k < n_off; ++k) {
        if (!(d[k] >= 0) || d[k] > (double)n) return false;
        off[k] = (int64_t)d[k];
    }
    return true;
}

// addSampleBatch(h, Int32Array ids, Float64Array offsets): bpe_add_sample_batch, sample k =
// ids[offsets[k] .. offsets[k+1])
napi_value AddSampleBatch(napi_env env, napi_callback_info info) {
    napi_value argv[3];
    if (!get_args(env, info, 3, argv)) return throw_arg(env, "addSampleBatch(h, Int32Array, Float64Array)");
    void *ids = nullptr, *offd = nullptr;
    size_t n = 0, n_off = 0;
    if (!get_typed(env, argv[1], napi_int32_array, &ids, &n) ||
        !get_typed(env, argv[2], napi_float64_array, &offd, &n_off) || n_off < 1)
        return throw_arg(env, "addSampleBatch expects Int32Array ids and Float64Array offsets");
    std::vector<int64_t> off;
    if (!get_offsets(offd, n_off, n, off)) return throw_arg(env, "addSampleBatch expects offsets within the ids");
    if (bpe_add_sample_batch(get_ctx(env, argv[0]), static_cast<const int32_t *>(ids), off.data(),
                             (int64_t)n_off - 1) < 0)
        return throw_native(env, "bpe_add_sample_batch");
    return nullptr;
}

// restoreTextBatch(h, textEncoder, Uint16Array units, Float64Array offsets): bpe_restore_text_batch,
// text k = units[offsets[k] .. offsets[k+1]), every text one sample
napi_value RestoreTextBatch(napi_env env, napi_callback_info info) {
    napi_value argv[4];
    if (!get_args(env, info, 4, argv))
        return throw_arg(env, "restoreTextBatch(h, textEncoder, Uint16Array, Float64Array)");
    void *units = nullptr, *offd = nullptr;
    size_t n = 0, n_off = 0;
    if (!get_typed(env, argv[2], napi_uint16_array, &units, &n) ||
        !get_typed(env, argv[3], napi_float64_array, &offd, &n_off) || n_off < 1)
        return throw_arg(env, "restoreTextBatch expects Uint16Array units and Float64Array offsets");
    std::vector<int64_t> off;
    if (!get_offsets(offd, n_off, n, off)) return throw_arg(env, "restoreTextBatch expects offsets within the units");
    if (bpe_restore_text_batch(get_ctx(env, argv[0]), get_encoder(env, argv[1]), static_cast<const uint16_t *>(units),
                               off.data(), (int64_t)n_off - 1) < 0)
        return throw_native(env, "bpe_restore_text_batch");
    return nullptr;
}

napi_value Init(napi_env env, napi_value exports) {
    struct {
        const char *name;
        napi_callback cb;
    } fns[] = {
        {"addSampleBatch", AddSampleBatch},
        {"restoreTextBatch", RestoreTextBatch},
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
