// bpe_utf8_out_napi.cc — Node N-API addon of the ways out as UTF-8 bytes (bpe_decode_utf8_batch,
// bpe_export_utf8_batch, include/bpe.h "text out as UTF-8"): what BPETokenizer.decodeVectorBatchUtf8
// and corpusToTextBatchUtf8 call.  A module of its own beside bpe_utf8_napi.node (the ways in), over
// the same libbpe.so; it takes the decoder handles bpe_decode_napi.node's createDecoder makes and the
// engine handles bpe_napi.node's createEngine makes (napi_util.h DecoderHolder, EngineHolder).  Every
// function maps 1:1 onto a bpe_* entry point; errors become JS errors carrying bpe_last_error().
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

bpe_decoder *get_decoder(napi_env env, napi_value v) {
    void *p = nullptr;
    if (napi_get_value_external(env, v, &p) != napi_ok || !p) return nullptr;
    return static_cast<DecoderHolder *>(p)->d;   // (null after destroyDecoder)
}

bool is_nullish(napi_env env, napi_value v) {
    napi_valuetype t;
    return napi_typeof(env, v, &t) == napi_ok && (t == napi_null || t == napi_undefined);
}

// One Buffer of `need` bytes (*data: its memory) for a call to fill.
bool make_buffer(napi_env env, size_t need, napi_value *buf, void **data) {
    return napi_create_buffer(env, need, data, buf) == napi_ok;
}

// text k = whole[off[k] .. off[k+1]) as a Buffer over the same allocation (Buffer.prototype.subarray)
napi_value slices(napi_env env, napi_value whole, const std::vector<int64_t> &off) {
    napi_value sub, out;
    if (napi_get_named_property(env, whole, "subarray", &sub) != napi_ok) return nullptr;
    napi_create_array_with_length(env, off.size() - 1, &out);
    for (size_t k = 0; k + 1 < off.size(); ++k) {
        napi_value args[2], piece;
        napi_create_double(env, (double)off[k], &args[0]);
        napi_create_double(env, (double)off[k + 1], &args[1]);
        if (napi_call_function(env, whole, sub, 2, args, &piece) != napi_ok) return nullptr;
        napi_set_element(env, out, (uint32_t)k, piece);
    }
    return out;
}

// decodeUtf8Batch(dec, Int32Array values, Float64Array offsets[, kind]) -> array of Buffers
// (bpe_decode_utf8_batch: text k = values[offsets[k] .. offsets[k+1]); kind BPE_DECODE_VECTORS 1
// (default) or BPE_DECODE_IDS 0): the sizing call, then the bytes into one Buffer, sliced per text
napi_value DecodeUtf8Batch(napi_env env, napi_callback_info info) {
    napi_value argv[4];
    size_t argc = 4;
    if (napi_get_cb_info(env, info, &argc, argv, nullptr, nullptr) != napi_ok || argc < 3)
        return throw_arg(env, "decodeUtf8Batch(dec, Int32Array, Float64Array[, kind])");
    const int kind = argc >= 4 ? (int)get_i64(env, argv[3]) : BPE_DECODE_VECTORS;
    napi_typedarray_type t;
    size_t n = 0, n_off = 0, o = 0;
    void *vals = nullptr, *offd = nullptr;
    napi_value ab;
    if (napi_get_typedarray_info(env, argv[1], &t, &n, &vals, &ab, &o) != napi_ok || t != napi_int32_array)
        return throw_arg(env, "decodeUtf8Batch expects Int32Array values and Float64Array offsets within them");
    if (napi_get_typedarray_info(env, argv[2], &t, &n_off, &offd, &ab, &o) != napi_ok || t != napi_float64_array ||
        n_off < 1)
        return throw_arg(env, "decodeUtf8Batch expects Int32Array values and Float64Array offsets within them");
    std::vector<int64_t> off(n_off);
    for (size_t k = 0; k < n_off; ++k) {
        const double d = static_cast<const double *>(offd)[k];
        if (!(d >= 0) || d > (double)n)
            return throw_arg(env, "decodeUtf8Batch expects Int32Array values and Float64Array offsets within them");
        off[k] = (int64_t)d;
    }
    bpe_decoder *dec = get_decoder(env, argv[0]);
    const int64_t n_texts = (int64_t)n_off - 1;
    std::vector<int64_t> out_off(n_off, 0);
    int rc = bpe_decode_utf8_batch(dec, kind, static_cast<const int32_t *>(vals), off.data(), n_texts, nullptr, 0,
                                   out_off.data());
    if (rc < 0 && !(rc == BPE_ERR_ARG && out_off[(size_t)n_texts] > 0)) return throw_native(env, "bpe_decode_utf8_batch");
    const size_t need = (size_t)out_off[(size_t)n_texts];
    napi_value whole;
    void *data = nullptr;
    if (!make_buffer(env, need, &whole, &data)) return throw_arg(env, "decodeUtf8Batch: the bytes do not fit a Buffer");
    if (need && bpe_decode_utf8_batch(dec, kind, static_cast<const int32_t *>(vals), off.data(), n_texts,
                                      static_cast<uint8_t *>(data), (int64_t)need, out_off.data()) < 0)
        return throw_native(env, "bpe_decode_utf8_batch");
    napi_value out = slices(env, whole, out_off);
    return out ? out : throw_arg(env, "decodeUtf8Batch: Buffer.prototype.subarray failed");
}

// exportUtf8(h, decoder, idxOrNull) -> array of Buffers (bpe_export_utf8_batch: the samples' texts
// through the decoder, as UTF-8; null or undefined: every sample, else a Float64Array or Int32Array of
// sample indices): the sizing call, then the bytes into one Buffer, sliced per sample
napi_value ExportUtf8(napi_env env, napi_callback_info info) {
    napi_value argv[3];
    if (!get_args(env, info, 3, argv)) return throw_arg(env, "exportUtf8(h, decoder, Float64Array|null)");
    bpe_ctx *c = get_ctx(env, argv[0]);
    bpe_decoder *dec = get_decoder(env, argv[1]);
    if (!c) return throw_arg(env, "exportUtf8 expects an engine handle");
    std::vector<int64_t> idx;
    const bool all = is_nullish(env, argv[2]);
    int64_t n = 0;
    if (all) {
        if (bpe_corpus_size(c, &n, nullptr) < 0) return throw_native(env, "bpe_corpus_size");
    } else {
        napi_typedarray_type t;
        size_t len = 0, o = 0;
        void *data = nullptr;
        napi_value ab;
        if (napi_get_typedarray_info(env, argv[2], &t, &len, &data, &ab, &o) != napi_ok ||
            (t != napi_float64_array && t != napi_int32_array))
            return throw_arg(env, "exportUtf8 expects a Float64Array or Int32Array of sample indices, or null");
        idx.resize(len);
        for (size_t k = 0; k < len; ++k) {
            const double d = t == napi_float64_array ? static_cast<const double *>(data)[k]
                                                     : (double)static_cast<const int32_t *>(data)[k];
            if (!(d >= -1) || d > 9007199254740992.0 || d != (double)(int64_t)d)
                return throw_arg(env, "exportUtf8 expects a Float64Array or Int32Array of sample indices, or null");
            idx[k] = (int64_t)d;
        }
        n = (int64_t)len;
    }
    const int64_t one = 0;
    const int64_t *idx_p = all ? nullptr : (idx.empty() ? &one : idx.data());
    std::vector<int64_t> off((size_t)n + 1, 0);
    int rc = bpe_export_utf8_batch(c, dec, idx_p, n, nullptr, 0, off.data());
    if (rc < 0 && !(rc == BPE_ERR_ARG && dec && off[(size_t)n] > 0)) return throw_native(env, "bpe_export_utf8_batch");
    const size_t need = (size_t)off[(size_t)n];
    napi_value whole;
    void *data = nullptr;
    if (!make_buffer(env, need, &whole, &data)) return throw_arg(env, "exportUtf8: the bytes do not fit a Buffer");
    if (need && bpe_export_utf8_batch(c, dec, idx_p, n, static_cast<uint8_t *>(data), (int64_t)need, off.data()) < 0)
        return throw_native(env, "bpe_export_utf8_batch");
    napi_value out = slices(env, whole, off);
    return out ? out : throw_arg(env, "exportUtf8: Buffer.prototype.subarray failed");
}

napi_value Init(napi_env env, napi_value exports) {
    struct {
        const char *name;
        napi_callback cb;
    } fns[] = {
        {"decodeUtf8Batch", DecodeUtf8Batch},
        {"exportUtf8", ExportUtf8},
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
