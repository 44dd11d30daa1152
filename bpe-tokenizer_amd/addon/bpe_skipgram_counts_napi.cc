// bpe_skipgram_counts_napi.cc — Node N-API addon of the skip-gram pair counts
// (bpe_skipgram_counts_text_batch, bpe_skipgram_counts_utf8_batch, bpe_export_skipgram_counts,
// include/bpe.h "skip-gram pair counts"): what BPETokenizer.skipGramCountsBatch,
// skipGramCountsBatchUtf8 and corpusToSkipGramCounts call.  A module of its own over the same
// libbpe.so; it takes the text encoder handles bpe_text_napi.node's createTextEncoder makes and the
// engine handles bpe_napi.node's createEngine makes (napi_util.h TextEncoderHolder, EngineHolder).
// Every function maps 1:1 onto a bpe_* entry point (the sizing call, then the real one); errors become
// JS errors carrying bpe_last_error().  Counts come back in a Float64Array: exact to 2^53, as the
// reference's numbers are.
#define NAPI_VERSION 6
#include <node_api.h>

#include <cstdint>
#include <functional>
#include <vector>

#include "bpe.h"
#include "napi_util.h"

namespace {

bool is_nullish(napi_env env, napi_value v) {
    napi_valuetype t;
    return napi_typeof(env, v, &t) == napi_ok && (t == napi_null || t == napi_undefined);
}

template <typename Holder>
Holder *get_holder(napi_env env, napi_value v) {
    void *p = nullptr;
    if (napi_get_value_external(env, v, &p) != napi_ok || !p) return nullptr;
    return static_cast<Holder *>(p);
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

// call(targets, contexts, counts, cap, needed) -> rc: the sizing call, then the planes
// -> [Int32Array targets, Int32Array contexts, Float64Array counts]
napi_value sized(napi_env env, const char *what,
                 const std::function<int(int32_t *, int32_t *, int64_t *, int64_t, int64_t *)> &call) {
    int64_t need = 0;
    int rc = call(nullptr, nullptr, nullptr, 0, &need);
    if (rc < 0 && !(rc == BPE_ERR_ARG && need > 0)) return throw_native(env, what);
    const size_t u = (size_t)need;
    std::vector<int64_t> counts(u);
    napi_value ab_t, ab_c, ab_n, a_t, a_c, a_n, out;
    void *pt = nullptr, *pc = nullptr, *pn = nullptr;
    if (napi_create_arraybuffer(env, u * 4, &pt, &ab_t) != napi_ok ||
        napi_create_arraybuffer(env, u * 4, &pc, &ab_c) != napi_ok ||
        napi_create_arraybuffer(env, u * 8, &pn, &ab_n) != napi_ok)
        return throw_arg(env, "skip-gram counts: the planes do not fit an ArrayBuffer");
    if (u && call(static_cast<int32_t *>(pt), static_cast<int32_t *>(pc), counts.data(), need, &need) < 0)
        return throw_native(env, what);
    for (size_t k = 0; k < u; ++k) static_cast<double *>(pn)[k] = (double)counts[k];
    napi_create_typedarray(env, napi_int32_array, u, ab_t, 0, &a_t);
    napi_create_typedarray(env, napi_int32_array, u, ab_c, 0, &a_c);
    napi_create_typedarray(env, napi_float64_array, u, ab_n, 0, &a_n);
    napi_create_array_with_length(env, 3, &out);
    napi_set_element(env, out, 0, a_t);
    napi_set_element(env, out, 1, a_c);
    napi_set_element(env, out, 2, a_n);
    return out;
}

// skipGramCounts{Text,Utf8}Batch(enc, Uint16Array units | Uint8Array bytes, Float64Array offsets, window, dim[, kind])
// (text k = data[offsets[k] .. offsets[k+1]); kind BPE_ENCODE_VECTORS 1 (default) or BPE_ENCODE_IDS 0)
template <bool UTF8>
napi_value CountsBatch(napi_env env, napi_callback_info info) {
    napi_value argv[6];
    size_t argc = 6;
    if (napi_get_cb_info(env, info, &argc, argv, nullptr, nullptr) != napi_ok || argc < 5)
        return throw_arg(env, "skipGramCounts*Batch(enc, typed array, Float64Array, window, dim[, kind])");
    const int window = (int)get_i64(env, argv[3]), dim = (int)get_i64(env, argv[4]);
    const int kind = argc >= 6 ? (int)get_i64(env, argv[5]) : BPE_ENCODE_VECTORS;
    const void *data = nullptr;
    std::vector<int64_t> off;
    if (!get_batch(env, argv[1], UTF8 ? napi_uint8_array : napi_uint16_array, argv[2], &data, off))
        return throw_arg(env, UTF8 ? "skipGramCountsUtf8Batch expects Uint8Array bytes and Float64Array offsets within them"
                                   : "skipGramCountsTextBatch expects Uint16Array units and Float64Array offsets within them");
    TextEncoderHolder *h = get_holder<TextEncoderHolder>(env, argv[0]);
    bpe_encoder *enc = h ? h->e : nullptr;   // (null after destroyTextEncoder: every call then fails)
    const int64_t n = (int64_t)off.size() - 1;
    return sized(env, UTF8 ? "bpe_skipgram_counts_utf8_batch" : "bpe_skipgram_counts_text_batch",
                 [&](int32_t *t, int32_t *c, int64_t *k, int64_t cap, int64_t *need) {
                     return UTF8 ? bpe_skipgram_counts_utf8_batch(enc, kind, static_cast<const uint8_t *>(data), off.data(),
                                                                  n, window, dim, t, c, k, cap, need)
                                 : bpe_skipgram_counts_text_batch(enc, kind, static_cast<const uint16_t *>(data), off.data(),
                                                                  n, window, dim, t, c, k, cap, need);
                 });
}

// exportSkipGramCounts(h, kind, idxOrNull, indexOrNull, window, dim) (bpe_export_skipgram_counts: kind
// BPE_EXPORT_IDS 0 or BPE_EXPORT_VECTORS 1; null or undefined indices: every sample, else a Float64Array
// or Int32Array of sample indices; index: to_vector_index as an Int32Array with -1 for holes)
napi_value ExportSkipGramCounts(napi_env env, napi_callback_info info) {
    napi_value argv[6];
    if (!get_args(env, info, 6, argv))
        return throw_arg(env, "exportSkipGramCounts(h, kind, Float64Array|null, Int32Array|null, window, dim)");
    EngineHolder *h = get_holder<EngineHolder>(env, argv[0]);
    bpe_ctx *c = h ? h->c : nullptr;
    if (!c) return throw_arg(env, "exportSkipGramCounts expects an engine handle");
    const int kind = (int)get_i64(env, argv[1]);
    const int window = (int)get_i64(env, argv[4]), dim = (int)get_i64(env, argv[5]);
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
            return throw_arg(env, "exportSkipGramCounts expects a Float64Array or Int32Array of sample indices, or null");
        idx.resize(len);
        for (size_t k = 0; k < len; ++k) {
            const double d = t == napi_float64_array ? static_cast<const double *>(data)[k]
                                                     : (double)static_cast<const int32_t *>(data)[k];
            if (!(d >= -1) || d > 9007199254740992.0 || d != (double)(int64_t)d)
                return throw_arg(env, "exportSkipGramCounts expects a Float64Array or Int32Array of sample indices, or null");
            idx[k] = (int64_t)d;
        }
        n = (int64_t)len;
    }
    const int32_t *tvi = nullptr;
    int32_t n_index = 0;
    if (!is_nullish(env, argv[3])) {
        if (napi_get_typedarray_info(env, argv[3], &t, &len, &data, &ab, &o) != napi_ok || t != napi_int32_array ||
            len > 0x7FFFFFFF)
            return throw_arg(env, "exportSkipGramCounts expects the vector index as an Int32Array, or null");
        static const int32_t none = -1;
        tvi = len ? static_cast<const int32_t *>(data) : &none;
        n_index = (int32_t)len;
    }
    const int64_t one = 0;
    const int64_t *idx_p = all ? nullptr : (idx.empty() ? &one : idx.data());
    return sized(env, "bpe_export_skipgram_counts", [&](int32_t *tg, int32_t *cx, int64_t *k, int64_t cap, int64_t *need) {
        return bpe_export_skipgram_counts(c, kind, idx_p, n, tvi, n_index, window, dim, tg, cx, k, cap, need);
    });
}

napi_value Init(napi_env env, napi_value exports) {
    struct {
        const char *name;
        napi_callback cb;
    } fns[] = {
        {"skipGramCountsTextBatch", CountsBatch<false>},
        {"skipGramCountsUtf8Batch", CountsBatch<true>},
        {"exportSkipGramCounts", ExportSkipGramCounts},
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
