// bpe_text_napi.cc — Node N-API addon of the device encoder's text form (bpe_encoder_set_chars,
// bpe_encoder_set_vector_index, bpe_encode_text_batch, include/bpe.h): what js/native.js
// syncTextEncoder and BPETokenizer.encodeToVectorBatch call.  A module of its own beside
// bpe_napi.node and bpe_decode_napi.node, over the same libbpe.so, with a bpe_encoder of its own.
// Every function maps 1:1 onto a bpe_* entry point; errors become JS errors carrying bpe_last_error().
#define NAPI_VERSION 6
#include <node_api.h>

#include <cstdint>
#include <string>
#include <vector>

#include "bpe.h"
#include "napi_util.h"

namespace {

// An encoder handle behind a JS external (napi_util.h TextEncoderHolder: bpe_restore_napi.node reads
// it too).
using EncoderHolder = TextEncoderHolder;

void finalize_encoder(napi_env, void *data, void *) {
    EncoderHolder *h = static_cast<EncoderHolder *>(data);
    if (!h) return;
    if (h->e) bpe_encoder_destroy(h->e);
    delete h;
}

bpe_encoder *get_encoder(napi_env env, napi_value v) {
    void *p = nullptr;
    if (napi_get_value_external(env, v, &p) != napi_ok || !p) return nullptr;
    return static_cast<EncoderHolder *>(p)->e;   // (null after destroyTextEncoder: every call then fails)
}

// a typed array of the given type: its data and length
bool get_typed(napi_env env, napi_value v, napi_typedarray_type want, void **data, size_t *n) {
    napi_typedarray_type t;
    size_t o = 0;
    napi_value ab;
    return napi_get_typedarray_info(env, v, &t, n, data, &ab, &o) == napi_ok && t == want;
}

// createTextEncoder([device]) -> external handle
napi_value CreateTextEncoder(napi_env env, napi_callback_info info) {
    napi_value argv[1];
    size_t argc = 1;
    napi_get_cb_info(env, info, &argc, argv, nullptr, nullptr);
    const int device = argc >= 1 ? (int)get_i64(env, argv[0]) : 0;
    bpe_encoder *enc = nullptr;
    if (bpe_encoder_create(&enc, device) != BPE_OK) return throw_native(env, "bpe_encoder_create");
    EncoderHolder *h = new EncoderHolder();
    h->e = enc;
    napi_value ext;
    napi_create_external(env, h, finalize_encoder, nullptr, &ext);
    return ext;
}

// destroyTextEncoder(enc)
napi_value DestroyTextEncoder(napi_env env, napi_callback_info info) {
    napi_value argv[1];
    if (!get_args(env, info, 1, argv)) return throw_arg(env, "destroyTextEncoder(enc)");
    void *p = nullptr;
    if (napi_get_value_external(env, argv[0], &p) != napi_ok || !p) return throw_arg(env, "destroyTextEncoder(enc)");
    EncoderHolder *h = static_cast<EncoderHolder *>(p);
    if (h->e) bpe_encoder_destroy(h->e);
    h->e = nullptr;
    return nullptr;
}

// textEncoderAddMerges(enc, Int32Array abc): appends (a, b, c) triples in list order
napi_value TextEncoderAddMerges(napi_env env, napi_callback_info info) {
    napi_value argv[2];
    if (!get_args(env, info, 2, argv)) return throw_arg(env, "textEncoderAddMerges(enc, Int32Array)");
    void *abc = nullptr;
    size_t n = 0;
    if (!get_typed(env, argv[1], napi_int32_array, &abc, &n) || n % 3 != 0)
        return throw_arg(env, "textEncoderAddMerges expects (a, b, c) triples in an Int32Array");
    if (bpe_encoder_add_merges(get_encoder(env, argv[0]), static_cast<const int32_t *>(abc), (int64_t)(n / 3)) < 0)
        return throw_native(env, "bpe_encoder_add_merges");
    return nullptr;
}

// textEncoderClear(enc): drops the merges (the char table stays)
napi_value TextEncoderClear(napi_env env, napi_callback_info info) {
    napi_value argv[1];
    if (!get_args(env, info, 1, argv)) return throw_arg(env, "textEncoderClear(enc)");
    if (bpe_encoder_clear(get_encoder(env, argv[0])) < 0) return throw_native(env, "bpe_encoder_clear");
    return nullptr;
}

// textEncoderSetChars(enc, Uint32Array code_points, Int32Array ids): replaces the char table
napi_value TextEncoderSetChars(napi_env env, napi_callback_info info) {
    napi_value argv[3];
    if (!get_args(env, info, 3, argv)) return throw_arg(env, "textEncoderSetChars(enc, Uint32Array, Int32Array)");
    void *cps = nullptr, *ids = nullptr;
    size_t n = 0, m = 0;
    if (!get_typed(env, argv[1], napi_uint32_array, &cps, &n) || !get_typed(env, argv[2], napi_int32_array, &ids, &m) ||
        n != m)
        return throw_arg(env, "textEncoderSetChars expects a Uint32Array of code points and an Int32Array of ids");
    if (bpe_encoder_set_chars(get_encoder(env, argv[0]), static_cast<const uint32_t *>(cps),
                              static_cast<const int32_t *>(ids), (int64_t)n) < 0)
        return throw_native(env, "bpe_encoder_set_chars");
    return nullptr;
}

// textEncoderSetVectorIndex(enc, Int32Array to_vector_index | null): -1 marks a hole
napi_value TextEncoderSetVectorIndex(napi_env env, napi_callback_info info) {
    napi_value argv[2];
    if (!get_args(env, info, 2, argv)) return throw_arg(env, "textEncoderSetVectorIndex(enc, Int32Array | null)");
    napi_valuetype vt;
    napi_typeof(env, argv[1], &vt);
    if (vt == napi_null || vt == napi_undefined) {
        if (bpe_encoder_set_vector_index(get_encoder(env, argv[0]), nullptr, 0) < 0)
            return throw_native(env, "bpe_encoder_set_vector_index");
        return nullptr;
    }
    void *idx = nullptr;
    size_t n = 0;
    if (!get_typed(env, argv[1], napi_int32_array, &idx, &n) || n > (size_t)BPE_MAX_VOCAB)
        return throw_arg(env, "textEncoderSetVectorIndex expects an Int32Array with one entry per token id");
    const int32_t none = -1;   // (an empty index is not "no index")
    if (bpe_encoder_set_vector_index(get_encoder(env, argv[0]), n ? static_cast<const int32_t *>(idx) : &none,
                                     (int32_t)n) < 0)
        return throw_native(env, "bpe_encoder_set_vector_index");
    return nullptr;
}

// encodeTextBatch(enc, Uint16Array units, Float64Array offsets[, kind]) -> [Int32Array values,
// Float64Array offsets] (bpe_encode_text_batch: text k = units[offsets[k] .. offsets[k+1]); kind
// BPE_ENCODE_VECTORS 1 (default) or BPE_ENCODE_IDS 0)
napi_value EncodeTextBatch(napi_env env, napi_callback_info info) {
    napi_value argv[4];
    size_t argc = 4;
    if (napi_get_cb_info(env, info, &argc, argv, nullptr, nullptr) != napi_ok || argc < 3)
        return throw_arg(env, "encodeTextBatch(enc, Uint16Array, Float64Array[, kind])");
    const int kind = argc >= 4 ? (int)get_i64(env, argv[3]) : BPE_ENCODE_VECTORS;
    void *units = nullptr, *offd = nullptr;
    size_t n = 0, n_off = 0;
    if (!get_typed(env, argv[1], napi_uint16_array, &units, &n) ||
        !get_typed(env, argv[2], napi_float64_array, &offd, &n_off) || n_off < 1)
        return throw_arg(env, "encodeTextBatch expects Uint16Array units and Float64Array offsets");
    std::vector<int64_t> off(n_off);
    const double *d = static_cast<const double *>(offd);
    for (size_t k = 0; k < n_off; ++k) {
        if (!(d[k] >= 0) || d[k] > (double)n)
            return throw_arg(env, "encodeTextBatch expects offsets within the units");
        off[k] = (int64_t)d[k];
    }
    const int64_t n_texts = (int64_t)n_off - 1;
    std::vector<int32_t> vals(n ? n : 1);
    std::vector<int64_t> out_off(n_off, 0);
    if (bpe_encode_text_batch(get_encoder(env, argv[0]), kind, static_cast<const uint16_t *>(units), off.data(),
                              n_texts, vals.data(), (int64_t)n, out_off.data()) < 0)
        return throw_native(env, "bpe_encode_text_batch");
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
        {"createTextEncoder", CreateTextEncoder}, {"destroyTextEncoder", DestroyTextEncoder},
        {"textEncoderAddMerges", TextEncoderAddMerges}, {"textEncoderClear", TextEncoderClear},
        {"textEncoderSetChars", TextEncoderSetChars}, {"textEncoderSetVectorIndex", TextEncoderSetVectorIndex},
        {"encodeTextBatch", EncodeTextBatch},
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
