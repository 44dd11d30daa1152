// bpe_decode_napi.cc — Node N-API addon of the device decoder (bpe_decoder_* / bpe_decode_batch,
// include/bpe.h): what js/native.js syncDecoder and BPETokenizer.decodeVectorBatch call.  A module of
// its own beside bpe_napi.node (the engine and the encoder), over the same libbpe.so.  Every function
// maps 1:1 onto a bpe_* entry point; errors become JS errors carrying bpe_last_error().
#define NAPI_VERSION 6
#include <node_api.h>

#include <cstdint>
#include <string>
#include <vector>

#include "bpe.h"
#include "napi_util.h"

namespace {

// A decoder handle (bpe_decoder_*: the vocabulary's chars on the device, decodeVector /
// decodeTokens core.ts:447-471 for batches) behind a JS external.  destroyDecoder() frees it at
// once; the holder goes with the external's finalizer (napi_util.h DecoderHolder).

void finalize_decoder(napi_env, void *data, void *) {
    DecoderHolder *h = static_cast<DecoderHolder *>(data);
    if (!h) return;
    if (h->d) bpe_decoder_destroy(h->d);
    delete h;
}

bpe_decoder *get_decoder(napi_env env, napi_value v) {
    void *p = nullptr;
    if (napi_get_value_external(env, v, &p) != napi_ok || !p) return nullptr;
    return static_cast<DecoderHolder *>(p)->d;   // (null after destroyDecoder: every call then fails)
}

// createDecoder([device]) -> external handle
napi_value CreateDecoder(napi_env env, napi_callback_info info) {
    napi_value argv[1];
    size_t argc = 1;
    napi_get_cb_info(env, info, &argc, argv, nullptr, nullptr);
    const int device = argc >= 1 ? (int)get_i64(env, argv[0]) : 0;
    bpe_decoder *dec = nullptr;
    if (bpe_decoder_create(&dec, device) != BPE_OK) return throw_native(env, "bpe_decoder_create");
    DecoderHolder *h = new DecoderHolder();
    h->d = dec;
    napi_value ext;
    napi_create_external(env, h, finalize_decoder, nullptr, &ext);
    return ext;
}

// destroyDecoder(dec)
napi_value DestroyDecoder(napi_env env, napi_callback_info info) {
    napi_value argv[1];
    if (!get_args(env, info, 1, argv)) return throw_arg(env, "destroyDecoder(dec)");
    void *p = nullptr;
    if (napi_get_value_external(env, argv[0], &p) != napi_ok || !p) return throw_arg(env, "destroyDecoder(dec)");
    DecoderHolder *h = static_cast<DecoderHolder *>(p);
    if (h->d) bpe_decoder_destroy(h->d);
    h->d = nullptr;
    return nullptr;
}

// decoderClear(dec)
napi_value DecoderClear(napi_env env, napi_callback_info info) {
    napi_value argv[1];
    if (!get_args(env, info, 1, argv)) return throw_arg(env, "decoderClear(dec)");
    if (bpe_decoder_clear(get_decoder(env, argv[0])) < 0) return throw_native(env, "bpe_decoder_clear");
    return nullptr;
}

// Float64Array offsets -> int64, each within [0, limit] (order is checked by the library)
bool get_offsets(napi_env env, napi_value v, size_t limit, std::vector<int64_t> *off) {
    napi_typedarray_type t;
    size_t n = 0, o = 0;
    void *data = nullptr;
    napi_value ab;
    if (napi_get_typedarray_info(env, v, &t, &n, &data, &ab, &o) != napi_ok || t != napi_float64_array || n < 1)
        return false;
    off->resize(n);
    const double *d = static_cast<const double *>(data);
    for (size_t k = 0; k < n; ++k) {
        if (!(d[k] >= 0) || d[k] > (double)limit) return false;
        (*off)[k] = (int64_t)d[k];
    }
    return true;
}

// decoderAddTokens(dec, Uint16Array units, Float64Array offsets): appends char tokens, token k's
// chars being units[offsets[k] .. offsets[k+1])
napi_value DecoderAddTokens(napi_env env, napi_callback_info info) {
    napi_value argv[3];
    if (!get_args(env, info, 3, argv)) return throw_arg(env, "decoderAddTokens(dec, Uint16Array, Float64Array)");
    napi_typedarray_type t;
    size_t n = 0, o = 0;
    void *units = nullptr;
    napi_value ab;
    std::vector<int64_t> off;
    if (napi_get_typedarray_info(env, argv[1], &t, &n, &units, &ab, &o) != napi_ok || t != napi_uint16_array ||
        !get_offsets(env, argv[2], n, &off))
        return throw_arg(env, "decoderAddTokens expects Uint16Array units and Float64Array offsets within them");
    if (bpe_decoder_add_tokens(get_decoder(env, argv[0]), static_cast<const uint16_t *>(units), off.data(),
                               (int64_t)off.size() - 1) < 0)
        return throw_native(env, "bpe_decoder_add_tokens");
    return nullptr;
}

// decoderAddMerges(dec, Int32Array abc): appends merged tokens, chars[c] = chars[a] + chars[b]
napi_value DecoderAddMerges(napi_env env, napi_callback_info info) {
    napi_value argv[2];
    if (!get_args(env, info, 2, argv)) return throw_arg(env, "decoderAddMerges(dec, Int32Array)");
    napi_typedarray_type t;
    size_t n = 0, o = 0;
    void *abc = nullptr;
    napi_value ab;
    if (napi_get_typedarray_info(env, argv[1], &t, &n, &abc, &ab, &o) != napi_ok ||
        t != napi_int32_array || n % 3 != 0)
        return throw_arg(env, "decoderAddMerges expects (a, b, c) triples in an Int32Array");
    if (bpe_decoder_add_merges(get_decoder(env, argv[0]), static_cast<const int32_t *>(abc),
                               (int64_t)(n / 3)) < 0)
        return throw_native(env, "bpe_decoder_add_merges");
    return nullptr;
}

// decoderSetVectorIndex(dec, Int32Array from_vector_index | null)
napi_value DecoderSetVectorIndex(napi_env env, napi_callback_info info) {
    napi_value argv[2];
    if (!get_args(env, info, 2, argv)) return throw_arg(env, "decoderSetVectorIndex(dec, Int32Array | null)");
    napi_valuetype vt;
    napi_typeof(env, argv[1], &vt);
    if (vt == napi_null || vt == napi_undefined) {
        if (bpe_decoder_set_vector_index(get_decoder(env, argv[0]), nullptr, 0) < 0)
            return throw_native(env, "bpe_decoder_set_vector_index");
        return nullptr;
    }
    napi_typedarray_type t;
    size_t n = 0, o = 0;
    void *idx = nullptr;
    napi_value ab;
    if (napi_get_typedarray_info(env, argv[1], &t, &n, &idx, &ab, &o) != napi_ok || t != napi_int32_array ||
        n > (size_t)BPE_MAX_VOCAB)
        return throw_arg(env, "decoderSetVectorIndex expects an Int32Array of token ids");
    const int32_t none = 0;   // (an empty index is not "no index")
    if (bpe_decoder_set_vector_index(get_decoder(env, argv[0]), n ? static_cast<const int32_t *>(idx) : &none,
                                     (int32_t)n) < 0)
        return throw_native(env, "bpe_decoder_set_vector_index");
    return nullptr;
}

// decodeBatch(dec, Int32Array values, Float64Array offsets[, kind]) -> array of strings
// (bpe_decode_batch: text k = values[offsets[k] .. offsets[k+1]); kind BPE_DECODE_VECTORS 1
// (default) or BPE_DECODE_IDS 0): the sizing call, then the units, cut into JS strings
napi_value DecodeBatch(napi_env env, napi_callback_info info) {
    napi_value argv[4];
    size_t argc = 4;
    if (napi_get_cb_info(env, info, &argc, argv, nullptr, nullptr) != napi_ok || argc < 3)
        return throw_arg(env, "decodeBatch(dec, Int32Array, Float64Array[, kind])");
    const int kind = argc >= 4 ? (int)get_i64(env, argv[3]) : BPE_DECODE_VECTORS;
    napi_typedarray_type t;
    size_t n = 0, o = 0;
    void *vals = nullptr;
    napi_value ab;
    std::vector<int64_t> off;
    if (napi_get_typedarray_info(env, argv[1], &t, &n, &vals, &ab, &o) != napi_ok || t != napi_int32_array ||
        !get_offsets(env, argv[2], n, &off))
        return throw_arg(env, "decodeBatch expects Int32Array values and Float64Array offsets within them");
    bpe_decoder *dec = get_decoder(env, argv[0]);
    const int64_t n_texts = (int64_t)off.size() - 1;
    std::vector<int64_t> out_off(off.size(), 0);
    std::vector<uint16_t> units;
    int rc = bpe_decode_batch(dec, kind, static_cast<const int32_t *>(vals), off.data(), n_texts, nullptr, 0,
                              out_off.data());
    if (rc == BPE_ERR_ARG && out_off[n_texts] > 0) {
        units.resize((size_t)out_off[n_texts]);
        rc = bpe_decode_batch(dec, kind, static_cast<const int32_t *>(vals), off.data(), n_texts, units.data(),
                              (int64_t)units.size(), out_off.data());
    }
    if (rc < 0) return throw_native(env, "bpe_decode_batch");
    napi_value out;
    napi_create_array_with_length(env, (size_t)n_texts, &out);
    if (units.empty()) units.push_back(0);   // (a valid pointer for empty strings)
    for (int64_t k = 0; k < n_texts; ++k) {
        napi_value s;
        if (napi_create_string_utf16(env, reinterpret_cast<const char16_t *>(units.data()) + out_off[k],
                                     (size_t)(out_off[k + 1] - out_off[k]), &s) != napi_ok)
            return throw_arg(env, "decodeBatch: a text does not fit a JS string");
        napi_set_element(env, out, (uint32_t)k, s);
    }
    return out;
}

napi_value Init(napi_env env, napi_value exports) {
    struct {
        const char *name;
        napi_callback cb;
    } fns[] = {
        {"createDecoder", CreateDecoder}, {"destroyDecoder", DestroyDecoder},
        {"decoderClear", DecoderClear}, {"decoderAddTokens", DecoderAddTokens},
        {"decoderAddMerges", DecoderAddMerges}, {"decoderSetVectorIndex", DecoderSetVectorIndex},
        {"decodeBatch", DecodeBatch},
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
