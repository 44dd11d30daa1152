// bpe_skipgram_napi.cc — Node N-API addon of the skip-gram pairs (bpe_skipgram_text_batch,
// bpe_skipgram_utf8_batch, bpe_export_skipgram, include/bpe.h "skip-gram pairs"): what
// BPETokenizer.skipGramBatch, skipGramBatchUtf8 and corpusToSkipGramBatch call.  A module of its own
// over the same libbpe.so; it takes the text encoder handles bpe_text_napi.node's createTextEncoder
// makes and the engine handles bpe_napi.node's createEngine makes (napi_util.h TextEncoderHolder,
// EngineHolder).  Every function maps 1:1 onto a bpe_* entry point (the sizing call, then the real
// one); errors become JS errors carrying bpe_last_error().
#define NAPI_VERSION 6
#include <node_api.h>

#include <cstdint>
#include <functional>
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

bool is_nullish(napi_env env, napi_value v) {
    napi_valuetype t;
    return napi_typeof(env, v, &t) == napi_ok && (t == napi_null || t == napi_undefined);
}

// (typed array of `want` elements, Float64Array offsets within [0, its length]) -> data and int64 offsets
bool get_batch(napi_env env, napi_value v_data, napi_typedarray_type want, napi_value v_off, const void **data,
               std::vector<int64_t> &off) {
    napi_typedarray_type t;
    size_t n = 0, n_off = 0, o = 0;
    void *p = nullptr, *offd = nullptr;
    napi_value ab;
    if (napi_get_typedarray_info(env, v_data, &t, &n, &p, &ab, &o) != napi_ok || t != want) return false;
    if (napi_get_typedarray_info(env, v_off, &t, &n_off, &offd, &ab, &o) != napi_ok || t != napi_float64_array ||
        n_off < 1)
        return false;
    off.resize(n_off);
    const double *d = static_cast<const double *>(offd);
    for (size_t k = 0; k < n_off; ++k) {
        if (!(d[k] >= 0) || d[k] > (double)n) return false;
        off[k] = (int64_t)d[k];
    }
    *data = p;
    return true;
}

// call(targets, contexts, cap, pair_off) -> rc: the sizing call, then the pairs into two Int32Arrays
// -> [Int32Array targets, Int32Array contexts, Float64Array offsets]
napi_value sized(napi_env env, const char *what, int64_t n,
                 const std::function<int(int32_t *, int32_t *, int64_t, int64_t *)> &call) {
    std::vector<int64_t> off((size_t)n + 1, 0);
    int rc = call(nullptr, nullptr, 0, off.data());
    if (rc < 0 && !(rc == BPE_ERR_ARG && off[(size_t)n] > 0)) return throw_native(env, what);
    const size_t need = (size_t)off[(size_t)n];
    napi_value ab_t, ab_c, ab_o, a_t, a_c, a_o, out;
    void *pt = nullptr, *pc = nullptr, *po = nullptr;
    if (napi_create_arraybuffer(env, need * 4, &pt, &ab_t) != napi_ok ||
        napi_create_arraybuffer(env, need * 4, &pc, &ab_c) != napi_ok ||
        napi_create_arraybuffer(env, ((size_t)n + 1) * 8, &po, &ab_o) != napi_ok)
        return throw_arg(env, "skip-gram: the pairs do not fit an ArrayBuffer");
    if (need && call(static_cast<int32_t *>(pt), static_cast<int32_t *>(pc), (int64_t)need, off.data()) < 0)
        return throw_native(env, what);
    for (size_t k = 0; k < off.size(); ++k) static_cast<double *>(po)[k] = (double)off[k];
    napi_create_typedarray(env, napi_int32_array, need, ab_t, 0, &a_t);
    napi_create_typedarray(env, napi_int32_array, need, ab_c, 0, &a_c);
    napi_create_typedarray(env, napi_float64_array, (size_t)n + 1, ab_o, 0, &a_o);
    napi_create_array_with_length(env, 3, &out);
    napi_set_element(env, out, 0, a_t);
    napi_set_element(env, out, 1, a_c);
    napi_set_element(env, out, 2, a_o);
    return out;
}

// skipGramTextBatch(enc, Uint16Array units, Float64Array offsets, window[, kind]) (bpe_skipgram_text_batch:
// text k = units[offsets[k] .. offsets[k+1]); kind BPE_ENCODE_VECTORS 1 (default) or BPE_ENCODE_IDS 0)
napi_value SkipGramTextBatch(napi_env env, napi_callback_info info) {
    napi_value argv[5];
    size_t argc = 5;
    if (napi_get_cb_info(env, info, &argc, argv, nullptr, nullptr) != napi_ok || argc < 4)
        return throw_arg(env, "skipGramTextBatch(enc, Uint16Array, Float64Array, window[, kind])");
    const int window = (int)get_i64(env, argv[3]);
    const int kind = argc >= 5 ? (int)get_i64(env, argv[4]) : BPE_ENCODE_VECTORS;
    const void *units = nullptr;
    std::vector<int64_t> off;
    if (!get_batch(env, argv[1], napi_uint16_array, argv[2], &units, off))
        return throw_arg(env, "skipGramTextBatch expects Uint16Array units and Float64Array offsets within them");
    bpe_encoder *enc = get_encoder(env, argv[0]);
    const int64_t n = (int64_t)off.size() - 1;
    return sized(env, "bpe_skipgram_text_batch", n, [&](int32_t *t, int32_t *c, int64_t cap, int64_t *po) {
        return bpe_skipgram_text_batch(enc, kind, static_cast<const uint16_t *>(units), off.data(), n, window, t, c, cap, po);
    });
}

// skipGramUtf8Batch(enc, Uint8Array bytes, Float64Array offsets, window[, kind]): bpe_skipgram_utf8_batch
napi_value SkipGramUtf8Batch(napi_env env, napi_callback_info info) {
    napi_value argv[5];
    size_t argc = 5;
    if (napi_get_cb_info(env, info, &argc, argv, nullptr, nullptr) != napi_ok || argc < 4)
        return throw_arg(env, "skipGramUtf8Batch(enc, Uint8Array, Float64Array, window[, kind])");
    const int window = (int)get_i64(env, argv[3]);
    const int kind = argc >= 5 ? (int)get_i64(env, argv[4]) : BPE_ENCODE_VECTORS;
    const void *bytes = nullptr;
    std::vector<int64_t> off;
    if (!get_batch(env, argv[1], napi_uint8_array, argv[2], &bytes, off))
        return throw_arg(env, "skipGramUtf8Batch expects Uint8Array bytes and Float64Array offsets within them");
    bpe_encoder *enc = get_encoder(env, argv[0]);
    const int64_t n = (int64_t)off.size() - 1;
    return sized(env, "bpe_skipgram_utf8_batch", n, [&](int32_t *t, int32_t *c, int64_t cap, int64_t *po) {
        return bpe_skipgram_utf8_batch(enc, kind, static_cast<const uint8_t *>(bytes), off.data(), n, window, t, c, cap, po);
    });
}

// exportSkipGram(h, kind, idxOrNull, indexOrNull, window) (bpe_export_skipgram: kind BPE_EXPORT_IDS 0 or
// BPE_EXPORT_VECTORS 1; null or undefined indices: every sample, else a Float64Array or Int32Array of
// sample indices; index: to_vector_index as an Int32Array with -1 for holes, for the vectors)
napi_value ExportSkipGram(napi_env env, napi_callback_info info) {
    napi_value argv[5];
    if (!get_args(env, info, 5, argv))
        return throw_arg(env, "exportSkipGram(h, kind, Float64Array|null, Int32Array|null, window)");
    bpe_ctx *c = get_ctx(env, argv[0]);
    if (!c) return throw_arg(env, "exportSkipGram expects an engine handle");
    const int kind = (int)get_i64(env, argv[1]);
    const int window = (int)get_i64(env, argv[4]);
    std::vector<int64_t> idx;
    const bool all = is_nullish(env, argv[2]);
    int64_t n = 0;
    napi_typedarray_type t;
    size_t len = 0, o = 0;
    void *data = nullptr;
    napi_value ab;
    if (all) {
        if (bpe_corpus_size(c, &n, nullptr) < 0) return throw_native(env, "bpe_corpus_size");
    } else {
        if (napi_get_typedarray_info(env, argv[2], &t, &len, &data, &ab, &o) != napi_ok ||
            (t != napi_float64_array && t != napi_int32_array))
            return throw_arg(env, "exportSkipGram expects a Float64Array or Int32Array of sample indices, or null");
        idx.resize(len);
        for (size_t k = 0; k < len; ++k) {
            const double d = t == napi_float64_array ? static_cast<const double *>(data)[k]
                                                     : (double)static_cast<const int32_t *>(data)[k];
            if (!(d >= -1) || d > 9007199254740992.0 || d != (double)(int64_t)d)
                return throw_arg(env, "exportSkipGram expects a Float64Array or Int32Array of sample indices, or null");
            idx[k] = (int64_t)d;
        }
        n = (int64_t)len;
    }
    const int32_t *tvi = nullptr;
    int32_t n_index = 0;
    if (!is_nullish(env, argv[3])) {
        if (napi_get_typedarray_info(env, argv[3], &t, &len, &data, &ab, &o) != napi_ok || t != napi_int32_array ||
            len > 0x7FFFFFFF)
            return throw_arg(env, "exportSkipGram expects the vector index as an Int32Array, or null");
        static const int32_t none = -1;
        tvi = len ? static_cast<const int32_t *>(data) : &none;
        n_index = (int32_t)len;
    }
    const int64_t one = 0;
    const int64_t *idx_p = all ? nullptr : (idx.empty() ? &one : idx.data());
    return sized(env, "bpe_export_skipgram", n, [&](int32_t *tg, int32_t *cx, int64_t cap, int64_t *po) {
        return bpe_export_skipgram(c, kind, idx_p, n, tvi, n_index, window, tg, cx, cap, po);
    });
}

napi_value Init(napi_env env, napi_value exports) {
    struct {
        const char *name;
        napi_callback cb;
    } fns[] = {
        {"skipGramTextBatch", SkipGramTextBatch},
        {"skipGramUtf8Batch", SkipGramUtf8Batch},
        {"exportSkipGram", ExportSkipGram},
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
