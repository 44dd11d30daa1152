// bpe_lines_napi.cc — Node N-API addon of the corpus helpers on the device (bpe_add_lines_batch,
// bpe_add_lines_utf8_batch, bpe_restore_lines_batch, bpe_restore_lines_utf8_batch, include/bpe.h
// "lines as samples"): what BPETokenizer.addLinesToCorpusBatch, addLinesToCorpusBatchUtf8,
// restoreLinesToCorpusBatch and restoreLinesToCorpusBatchUtf8 call.  A module of its own beside
// bpe_napi.node, over the same libbpe.so; it takes the engine handles bpe_napi.node's createEngine
// makes and the text encoder handles bpe_text_napi.node's createTextEncoder makes (napi_util.h
// EngineHolder, TextEncoderHolder).  Every function maps 1:1 onto a bpe_* entry point; errors become
// JS errors carrying bpe_last_error().  mode: BPE_LINES_TRIM 0, BPE_LINES_KEEP 1, BPE_LINES_FILE 2.
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

// (a typed array of `want` elements, Float64Array offsets within it) -> its data and int64 offsets
bool get_batch(napi_env env, napi_value v_data, napi_value v_off, napi_typedarray_type want, const void **data,
               std::vector<int64_t> &off) {
    napi_typedarray_type t;
    size_t n = 0, n_off = 0, o = 0;
    void *d = nullptr, *offd = nullptr;
    napi_value ab;
    if (napi_get_typedarray_info(env, v_data, &t, &n, &d, &ab, &o) != napi_ok || t != want) return false;
    if (napi_get_typedarray_info(env, v_off, &t, &n_off, &offd, &ab, &o) != napi_ok || t != napi_float64_array ||
        n_off < 1)
        return false;
    off.resize(n_off);
    const double *x = static_cast<const double *>(offd);
    for (size_t k = 0; k < n_off; ++k) {
        if (!(x[k] >= 0) || x[k] > (double)n) return false;
        off[k] = (int64_t)x[k];
    }
    *data = d;
    return true;
}

// [Uint32Array newChars, Float64Array hist], as bpe_ingest_napi.node's addTextBatch returns them
napi_value added(napi_env env, bpe_ctx *ctx, const std::vector<uint32_t> &fresh, int64_t n_new,
                 const std::vector<int64_t> &hist) {
    int32_t nt = 0;
    if (bpe_num_tokens(ctx, &nt) < 0) return throw_native(env, "bpe_num_tokens");
    napi_value ab_new, ab_hist, a_new, a_hist, out;
    void *pn = nullptr, *ph = nullptr;
    napi_create_arraybuffer(env, (size_t)n_new * 4, &pn, &ab_new);
    napi_create_arraybuffer(env, (size_t)nt * 8, &ph, &ab_hist);
    for (int64_t i = 0; i < n_new; ++i) static_cast<uint32_t *>(pn)[i] = fresh[(size_t)i];
    for (int32_t i = 0; i < nt; ++i) static_cast<double *>(ph)[i] = (double)hist[(size_t)i];
    napi_create_typedarray(env, napi_uint32_array, (size_t)n_new, ab_new, 0, &a_new);
    napi_create_typedarray(env, napi_float64_array, (size_t)nt, ab_hist, 0, &a_hist);
    napi_create_array_with_length(env, 2, &out);
    napi_set_element(env, out, 0, a_new);
    napi_set_element(env, out, 1, a_hist);
    return out;
}

// addLinesBatch(h, mode, Uint16Array units, Float64Array offsets) and
// addLinesUtf8Batch(h, mode, Uint8Array bytes, Float64Array offsets) -> [newChars, hist]
// (bpe_add_lines_batch, bpe_add_lines_utf8_batch: text k = data[offsets[k] .. offsets[k+1]), split
// into samples by the helper `mode` names)
template <bool UTF8>
napi_value AddLines(napi_env env, napi_callback_info info) {
    napi_value argv[4];
    if (!get_args(env, info, 4, argv))
        return throw_arg(env, UTF8 ? "addLinesUtf8Batch(h, mode, Uint8Array, Float64Array)"
                                   : "addLinesBatch(h, mode, Uint16Array, Float64Array)");
    bpe_ctx *ctx = get_ctx(env, argv[0]);
    const int mode = (int)get_i64(env, argv[1]);
    const void *data = nullptr;
    std::vector<int64_t> off;
    if (!get_batch(env, argv[2], argv[3], UTF8 ? napi_uint8_array : napi_uint16_array, &data, off))
        return throw_arg(env, UTF8 ? "addLinesUtf8Batch expects Uint8Array bytes and Float64Array offsets within them"
                                   : "addLinesBatch expects Uint16Array units and Float64Array offsets within them");
    std::vector<uint32_t> fresh(BPE_MAX_VOCAB);
    std::vector<int64_t> hist(BPE_MAX_VOCAB);
    int64_t n_new = 0;
    const int64_t n = (int64_t)off.size() - 1;
    const int rc = UTF8 ? bpe_add_lines_utf8_batch(ctx, mode, static_cast<const uint8_t *>(data), off.data(), n,
                                                   fresh.data(), BPE_MAX_VOCAB, &n_new, hist.data(), BPE_MAX_VOCAB)
                        : bpe_add_lines_batch(ctx, mode, static_cast<const uint16_t *>(data), off.data(), n,
                                              fresh.data(), BPE_MAX_VOCAB, &n_new, hist.data(), BPE_MAX_VOCAB);
    if (rc < 0) return throw_native(env, UTF8 ? "bpe_add_lines_utf8_batch" : "bpe_add_lines_batch");
    return added(env, ctx, fresh, n_new, hist);
}

// restoreLinesBatch(h, textEncoder, mode, Uint16Array units, Float64Array offsets) and
// restoreLinesUtf8Batch(h, textEncoder, mode, Uint8Array bytes, Float64Array offsets)
// (bpe_restore_lines_batch, bpe_restore_lines_utf8_batch)
template <bool UTF8>
napi_value RestoreLines(napi_env env, napi_callback_info info) {
    napi_value argv[5];
    if (!get_args(env, info, 5, argv))
        return throw_arg(env, UTF8 ? "restoreLinesUtf8Batch(h, textEncoder, mode, Uint8Array, Float64Array)"
                                   : "restoreLinesBatch(h, textEncoder, mode, Uint16Array, Float64Array)");
    const int mode = (int)get_i64(env, argv[2]);
    const void *data = nullptr;
    std::vector<int64_t> off;
    if (!get_batch(env, argv[3], argv[4], UTF8 ? napi_uint8_array : napi_uint16_array, &data, off))
        return throw_arg(env, UTF8 ? "restoreLinesUtf8Batch expects Uint8Array bytes and Float64Array offsets within them"
                                   : "restoreLinesBatch expects Uint16Array units and Float64Array offsets within them");
    bpe_ctx *ctx = get_ctx(env, argv[0]);
    bpe_encoder *enc = get_encoder(env, argv[1]);
    const int64_t n = (int64_t)off.size() - 1;
    const int rc = UTF8 ? bpe_restore_lines_utf8_batch(ctx, enc, mode, static_cast<const uint8_t *>(data), off.data(), n)
                        : bpe_restore_lines_batch(ctx, enc, mode, static_cast<const uint16_t *>(data), off.data(), n);
    if (rc < 0) return throw_native(env, UTF8 ? "bpe_restore_lines_utf8_batch" : "bpe_restore_lines_batch");
    return nullptr;
}

napi_value Init(napi_env env, napi_value exports) {
    struct {
        const char *name;
        napi_callback cb;
    } fns[] = {
        {"addLinesBatch", AddLines<false>},
        {"addLinesUtf8Batch", AddLines<true>},
        {"restoreLinesBatch", RestoreLines<false>},
        {"restoreLinesUtf8Batch", RestoreLines<true>},
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
