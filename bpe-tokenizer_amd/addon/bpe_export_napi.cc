// bpe_export_napi.cc — Node N-API addon of the corpus export (bpe_export_samples,
// bpe_export_text_batch, include/bpe.h): what BPETokenizer's corpus_in_code getter, corpusToVectorBatch
// and corpusToTextBatch and BPETokenizerDB.syncRows call.  A module of its own beside bpe_napi.node,
// over the same libbpe.so; it takes the engine handles bpe_napi.node's createEngine makes and the
// decoder handles bpe_decode_napi.node's createDecoder makes (napi_util.h EngineHolder,
// DecoderHolder).  Every function maps 1:1 onto a bpe_* entry point; errors become JS errors carrying
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

bpe_decoder *get_decoder(napi_env env, napi_value v) {
    void *p = nullptr;
    if (napi_get_value_external(env, v, &p) != napi_ok || !p) return nullptr;
    return static_cast<DecoderHolder *>(p)->d;   // (null after destroyDecoder)
}

bool is_nullish(napi_env env, napi_value v) {
    napi_valuetype t;
    return napi_typeof(env, v, &t) == napi_ok && (t == napi_null || t == napi_undefined);
}

// The sample list of a call: null or undefined -> every sample (idx NULL, n = the sample count);
// else a Float64Array or Int32Array of sample indices.
bool get_indices(napi_env env, bpe_ctx *c, napi_value v, std::vector<int64_t> &idx, bool *all, int64_t *n) {
    *all = is_nullish(env, v);
    if (*all) {
        int64_t ns = 0;
        if (bpe_corpus_size(c, &ns, nullptr) < 0) return false;
        *n = ns;
        return true;
    }
    napi_typedarray_type t;
    size_t len = 0, o = 0;
    void *data = nullptr;
    napi_value ab;
    if (napi_get_typedarray_info(env, v, &t, &len, &data, &ab, &o) != napi_ok ||
        (t != napi_float64_array && t != napi_int32_array))
        return false;
    idx.resize(len);
    for (size_t k = 0; k < len; ++k) {
        const double d = t == napi_float64_array ? static_cast<const double *>(data)[k]
                                                 : (double)static_cast<const int32_t *>(data)[k];
        if (!(d >= -1) || d > 9007199254740992.0 || d != (double)(int64_t)d) return false;
        idx[k] = (int64_t)d;
    }
    *n = (int64_t)len;
    return true;
}

napi_value offsets_out(napi_env env, const std::vector<int64_t> &off) {
    napi_value ab, arr;
    void *data = nullptr;
    napi_create_arraybuffer(env, off.size() * sizeof(double), &data, &ab);
    for (size_t k = 0; k < off.size(); ++k) static_cast<double *>(data)[k] = (double)off[k];
    napi_create_typedarray(env, napi_float64_array, off.size(), ab, 0, &arr);
    return arr;
}

// exportSamples(h, kind, idxOrNull, toVectorIndexOrNull) -> [values, Float64Array offsets]
// (bpe_export_samples: kind BPE_EXPORT_IDS 0 and BPE_EXPORT_VECTORS 1 give an Int32Array,
// BPE_EXPORT_CODE 2 a Uint16Array of the samples' code units): the sizing call, then the values
// straight into the typed array's buffer
napi_value ExportSamples(napi_env env, napi_callback_info info) {
    napi_value argv[4];
    if (!get_args(env, info, 4, argv))
        return throw_arg(env, "exportSamples(h, kind, Float64Array|null, Int32Array|null)");
    bpe_ctx *c = get_ctx(env, argv[0]);
    const int kind = (int)get_i64(env, argv[1]);
    std::vector<int64_t> idx;
    bool all = false;
    int64_t n = 0;
    if (!c) return throw_arg(env, "exportSamples expects an engine handle");
    if (!get_indices(env, c, argv[2], idx, &all, &n))
        return throw_arg(env, "exportSamples expects a Float64Array or Int32Array of sample indices, or null");
    const int32_t *tvi = nullptr;
    int32_t n_index = 0;
    const int32_t none = 0;
    if (!is_nullish(env, argv[3])) {
        napi_typedarray_type t;
        size_t len = 0, o = 0;
        void *data = nullptr;
        napi_value ab;
        if (napi_get_typedarray_info(env, argv[3], &t, &len, &data, &ab, &o) != napi_ok || t != napi_int32_array)
            return throw_arg(env, "exportSamples expects an Int32Array to_vector_index, or null");
        tvi = len ? static_cast<const int32_t *>(data) : &none;
        n_index = (int32_t)len;
    }
    const int64_t one = 0;
    const int64_t *idx_p = all ? nullptr : (idx.empty() ? &one : idx.data());
    std::vector<int64_t> off((size_t)n + 1, 0);
    int rc = bpe_export_samples(c, kind, idx_p, n, tvi, n_index, nullptr, 0, off.data());
    if (rc < 0 && !(rc == BPE_ERR_ARG && off[(size_t)n] > 0)) return throw_native(env, "bpe_export_samples");
    const size_t need = (size_t)off[(size_t)n], esize = kind == BPE_EXPORT_CODE ? 2 : 4;
    napi_value ab, vals;
    void *data = nullptr;
    if (napi_create_arraybuffer(env, need * esize, &data, &ab) != napi_ok)
        return throw_arg(env, "exportSamples: the values do not fit an ArrayBuffer");
    if (need && bpe_export_samples(c, kind, idx_p, n, tvi, n_index, data, (int64_t)need, off.data()) < 0)
        return throw_native(env, "bpe_export_samples");
    napi_create_typedarray(env, kind == BPE_EXPORT_CODE ? napi_uint16_array : napi_int32_array, need, ab, 0, &vals);
    napi_value out;
    napi_create_array_with_length(env, 2, &out);
    napi_set_element(env, out, 0, vals);
    napi_set_element(env, out, 1, offsets_out(env, off));
    return out;
}

// exportText(h, decoder, idxOrNull) -> array of strings (bpe_export_text_batch: the samples' texts
// through the decoder): the sizing call, then the units, cut into JS strings
napi_value ExportText(napi_env env, napi_callback_info info) {
    napi_value argv[3];
    if (!get_args(env, info, 3, argv)) return throw_arg(env, "exportText(h, decoder, Float64Array|null)");
    bpe_ctx *c = get_ctx(env, argv[0]);
    bpe_decoder *dec = get_decoder(env, argv[1]);
    std::vector<int64_t> idx;
    bool all = false;
    int64_t n = 0;
    if (!c) return throw_arg(env, "exportText expects an engine handle");
    if (!get_indices(env, c, argv[2], idx, &all, &n))
        return throw_arg(env, "exportText expects a Float64Array or Int32Array of sample indices, or null");
    const int64_t one = 0;
    const int64_t *idx_p = all ? nullptr : (idx.empty() ? &one : idx.data());
    std::vector<int64_t> off((size_t)n + 1, 0);
    std::vector<uint16_t> units;
    int rc = bpe_export_text_batch(c, dec, idx_p, n, nullptr, 0, off.data());
    if (rc == BPE_ERR_ARG && dec && off[(size_t)n] > 0) {
        units.resize((size_t)off[(size_t)n]);
        rc = bpe_export_text_batch(c, dec, idx_p, n, units.data(), (int64_t)units.size(), off.data());
    }
    if (rc < 0) return throw_native(env, "bpe_export_text_batch");
    napi_value out;
    napi_create_array_with_length(env, (size_t)n, &out);
    if (units.empty()) units.push_back(0);   // (a valid pointer for empty strings)
    for (int64_t k = 0; k < n; ++k) {
        napi_value s;
        if (napi_create_string_utf16(env, reinterpret_cast<const char16_t *>(units.data()) + off[(size_t)k],
                                     (size_t)(off[(size_t)k + 1] - off[(size_t)k]), &s) != napi_ok)
            return throw_arg(env, "exportText: a text does not fit a JS string");
        napi_set_element(env, out, (uint32_t)k, s);
    }
    return out;
}

napi_value Init(napi_env env, napi_value exports) {
    struct {
        const char *name;
        napi_callback cb;
    } fns[] = {
        {"exportSamples", ExportSamples},
        {"exportText", ExportText},
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
