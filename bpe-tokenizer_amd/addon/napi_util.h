// napi_util.h — what the N-API modules (bpe_napi.cc, bpe_decode_napi.cc, bpe_text_napi.cc,
// bpe_ingest_napi.cc, bpe_restore_napi.cc, bpe_export_napi.cc) share: errors as JS exceptions carrying
// bpe_last_error(), argument access, and the engine, text encoder and decoder handles.
#pragma once
#include <node_api.h>

#include <cstdint>
#include <string>

#include "bpe.h"

namespace {

// What an engine handle (bpe_napi.node createEngine's JS external) points to; the modules that take
// such a handle read the context through it.
struct EngineHolder {
    bpe_ctx *c = nullptr;
};

// What a text encoder handle (bpe_text_napi.node createTextEncoder's JS external) points to.
// destroyTextEncoder() frees the encoder at once; the holder goes with the external's finalizer.
struct TextEncoderHolder {
    bpe_encoder *e = nullptr;
};

// What a decoder handle (bpe_decode_napi.node createDecoder's JS external) points to.
// destroyDecoder() frees the decoder at once; the holder goes with the external's finalizer.
struct DecoderHolder {
    bpe_decoder *d = nullptr;
};

napi_value throw_native(napi_env env, const char *what) {
    char buf[1024];
    bpe_last_error(buf, sizeof buf);
    std::string msg = buf[0] ? std::string(buf) : std::string("bpe native: ") + what + " failed";
    napi_throw_error(env, nullptr, msg.c_str());
    return nullptr;
}

napi_value throw_arg(napi_env env, const char *msg) {
    napi_throw_type_error(env, nullptr, msg);
    return nullptr;
}

bool get_args(napi_env env, napi_callback_info info, size_t want, napi_value *argv) {
    size_t argc = want;
    if (napi_get_cb_info(env, info, &argc, argv, nullptr, nullptr) != napi_ok) return false;
    return argc >= want;
}

inline int64_t get_i64(napi_env env, napi_value v) {
    int64_t x = 0;
    napi_get_value_int64(env, v, &x);
    return x;
}

}  // namespace
