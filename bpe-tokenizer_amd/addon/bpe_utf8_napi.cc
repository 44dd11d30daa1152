// bpe_utf8_napi.cc — Node N-API addon of the text pipelines from UTF-8 bytes (bpe_add_utf8_batch,
// bpe_restore_utf8_batch, bpe_encode_utf8_batch, include/bpe.h "text as UTF-8"): what
// BPETokenizer.addToCorpusBatchUtf8, restoreToCorpusBatchUtf8 and encodeToVectorBatchUtf8 call.  A
// module of its own beside bpe_napi.node, over the same libbpe.so; it takes the engine handles
// bpe_napi.node's createEngine makes and the text encoder handles bpe_text_napi.node's
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

// (Uint8Array bytes, Float64Array offsets within [0, bytes]) -> the bytes and int64 offsets
bool get_batch(napi_env env, napi_value v_bytes, napi_value v_off, const uint8_t **bytes, std::vector<int64_t> &off) {
    napi_typedarray_type t;
    size_t n = 0, n_off = 0, o = 0;
    void *data = nullptr, *offd = nullptr;
    napi_value ab;
    if (napi_get_typedarray_info(env, v_bytes, &t, &n, &data, &ab, &o) != napi_ok || t != napi_uint8_array) return false;
    if (napi_get_typedarray_info(env, v_off, &t, &n_off, &offd, &ab, &o) != napi_ok || t != napi_float64_array ||
        n_off < 1)
        return false;
    off.resize(n_off);
    const double *d = static_cast<const double *>(offd);
    for (size_t k = 0; k < n_off; ++k) {
        if (!(d[k] >= 0) || d[k] > (double)n) return false;
        off[k] = (int64_t)d[k];
    }
    *bytes = static_cast<const uint8_t *>(data);
    return true;
}

// addUtf8Batch(h, Uint8Array bytes, Float64Array offsets) -> [Uint32Array newChars, Float64Array hist]
// (bpe_add_utf8_batch: text k = bytes[offsets[k] .. offsets[k+1]), every text one sample; the outputs
// as bpe_ingest_napi.node's addTextBatch returns them)
napi_value AddUtf8Batch(napi_env env, napi_callback_info info) {
    napi_value argv[3];
    if (!get_args(env, info, 3, argv)) return throw_arg(env, "addUtf8Batch(h, Uint8Array, Float64Array)");
    bpe_ctx *ctx = get_ctx(env, argv[0]);
    const uint8_t *bytes = nullptr;
    std::vector<int64_t> off;
    if (!get_batch(env, argv[1], argv[2], &bytes, off))
        return throw_arg(env, "addUtf8Batch expects Uint8Array bytes and Float64Array offsets within them");
    std::vector<uint32_t> fresh(BPE_MAX_VOCAB);
    std::vector<int64_t> hist(BPE_MAX_VOCAB);
    int64_t n_new = 0;
    if (bpe_add_utf8_batch(ctx, bytes, off.data(), (int64_t)off.size() - 1, fresh.data(), BPE_MAX_VOCAB, &n_new,
                           hist.data(), BPE_MAX_VOCAB) < 0)
        return throw_native(env, "bpe_add_utf8_batch");
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

// restoreUtf8Batch(h, textEncoder, Uint8Array bytes, Float64Array offsets): bpe_restore_utf8_batch
napi_value RestoreUtf8Batch(napi_env env, napi_callback_info info) {
    napi_value argv[4];
    if (!get_args(env, info, 4, argv)) return throw_arg(env, "restoreUtf8Batch(h, textEncoder, Uint8Array, Float64Array)");
    const uint8_t *bytes = nullptr;
    std::vector<int64_t> off;
    if (!get_batch(env, argv[2], argv[3], &bytes, off))
        return throw_arg(env, "restoreUtf8Batch expects Uint8Array bytes and Float64Array offsets within them");
    if (bpe_restore_utf8_batch(get_ctx(env, argv[0]), get_encoder(env, argv[1]), bytes, off.data(),
                               (int64_t)off.size() - 1) < 0)
        return throw_native(env, "bpe_restore_utf8_batch");
    return nullptr;
}

// encodeUtf8Batch(enc, Uint8Array bytes, Float64Array offsets[, kind]) -> [Int32Array values,
// Float64Array offsets] (bpe_encode_utf8_batch; kind BPE_ENCODE_VECTORS 1 (default) or BPE_ENCODE_IDS 0)
napi_value EncodeUtf8Batch(napi_env env, napi_callback_info info) {
    napi_value argv[4];
    size_t argc = 4;
    if (napi_get_cb_info(env, info, &argc, argv, nullptr, nullptr) != napi_ok || argc < 3)
        return throw_arg(env, "encodeUtf8Batch(enc, Uint8Array, Float64Array[, kind])");
    const int kind = argc >= 4 ? (int)get_i64(env, argv[3]) : BPE_ENCODE_VECTORS;
    const uint8_t *bytes = nullptr;
    std::vector<int64_t> off;
    if (!get_batch(env, argv[1], argv[2], &bytes, off))
        return throw_arg(env, "encodeUtf8Batch expects Uint8Array bytes and Float64Array offsets within them");
    const size_t n_off = off.size();
    const int64_t n_texts = (int64_t)n_off - 1, total = off[n_off - 1] > off[0] ? off[n_off - 1] - off[0] : 0;
    std::vector<int32_t> vals((size_t)(total ? total : 1));   // (a text never grows: values <= units <= bytes)
    std::vector<int64_t> out_off(n_off, 0);
    if (bpe_encode_utf8_batch(get_encoder(env, argv[0]), kind, bytes, off.data(), n_texts, vals.data(), total,
                              out_off.data()) < 0)
        return throw_native(env, "bpe_encode_utf8_batch");
    const size_t n_out = (size_t)out_off[n_texts];
    napi_value ab_vals, ab_off, a_vals, a_off, out;
    void *pv = nullptr, *po = nullptr;
    napi_create_arraybuffer(env, n_out * 4, &pv, &ab_vals);
    napi_create_arraybuffer(env, n_off * 8, &po, &ab_off);
    for (size_t i = 0; i < n_out; ++i) static_cast<int32_t *>(pv)[i] = vals[i];
    for (size_t k = 0; k < n_off; ++k) static_cast<double *>(po)[k] = (double)out_off[k];
    napi_create_typedarray(env, napi_int32_array, n_out, ab_vals, 0, &a_vals);
    napi_create_typedarray(env, napi_float64_array, n_off, ab_off, 0, &a_off);
    napi_create_array_with_length(env, 2, &out);
    napi_set_element(env, out, 0, a_vals);
    napi_set_element(env, out, 1, a_off);
    return out;
}

napi_value Init(napi_env env, napi_value exports) {
    struct {
        const char *name;
        napi_callback cb;
    } fns[] = {
        {"addUtf8Batch", AddUtf8Batch},
        {"restoreUtf8Batch", RestoreUtf8Batch},
        {"encodeUtf8Batch", EncodeUtf8Batch},
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
