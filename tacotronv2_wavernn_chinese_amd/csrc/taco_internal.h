// What tacotron.hip shares with taco_gta.hip (host only): the handle, and the part of wrnn_taco_synthesize that follows its host-side
// checks and its copies of the text -- the launches -- so that another entry runs the very same kernels on buffers of its own.
#pragma once
#include <string>
#include <vector>

#include "handle_common.h"

struct TacoTensor {
    std::string name;
    std::vector<int64_t> shape;
    std::vector<float> data;   // empty until loaded
    size_t off = 0;            // floats, in the device image
    size_t count() const {
        size_t n = 1;
        for (int64_t e : shape) n *= (size_t)e;
        return n;
    }
};

struct wrnn_taco_handle {
    wrnn_taco_dims d{};
    bool ok = false;
    std::vector<TacoTensor> tensors;
    bool dirty = true;            // a tensor was loaded since the last upload
    float *img = nullptr;         // the device image: the tensors in table order, then the derived ones
    size_t img_cap = 0;
    size_t off_bn_enc = 0, off_bn_post = 0, off_loc_m = 0, off_att_bias = 0, off_proj_w = 0, off_proj_b = 0;
    WrnnScratch ws;               // the scratch of a call, grown on demand
    WrnnScratch gta_ws;           // wrnn_taco_gta_corpus's own: the text, the packed target and every intermediate output of a group
    int open_streams = 0;         // wrnn_taco_stream objects that read img
    bool destroyed = false;       // wrnn_taco_destroy came while streams were open: the last close frees the handle
    std::string err;
};

// Byte offsets of what a call keeps in scratch: ids, tx, the target's steps, seeds; two ping-pong activations; the LSTM input
// projections; memory; keys.  `end` is the first byte behind them (256-byte aligned).
struct TacoBufs {
    size_t ids, tx, gs, seeds, a0, a1, xp0, xp1, mem, keys, end;
};
TacoBufs taco_layout(const wrnn_taco_dims &d, int B, int Tx_max, int S);

// A call behind its checks: ids, tx, gs (with a target) and seeds are on the device at ws + o.*, or on their way there on the stream.
struct TacoRun {
    int B, Tx_max, S, gta_max, max_iters, dropout;
    char *ws;
    TacoBufs o;
    const float *gta;   // null, or (B, gta_max, num_mels)
    float *encoder;     // null, or as wrnn_taco_call's; the rest as wrnn_taco_call's, never null
    float *decoder, *mel_raw, *mel, *alignments, *stop;
    int32_t *max_attentions, *steps, *mel_frames;
};
// Zeroes the outputs and launches encoder, decoder, postnet and finish on `s`.  No host wait.
int taco_run(wrnn_taco_handle *h, hipStream_t s, const TacoRun &r);

// The host-side checks of wrnn_taco_synthesize, with its wording.
int taco_check_text(wrnn_taco_handle *h, int B, int Tx_max, const int32_t *ids_host, const int32_t *tx_host, const uint64_t *seeds_host);
int taco_check_symbols(wrnn_taco_handle *h, int B, int Tx_max, const int32_t *ids_host, const int32_t *tx_host);
int taco_check_decoder_lds(wrnn_taco_handle *h, int Tx_max);
// The one wording of "utterance b has tx symbols, outside 1 .. Tx_max": taco_check_symbols' refusal, also raised by wrnn_taco_gta_corpus.
int taco_refuse_length(wrnn_taco_handle *h, int b, int tx, int Tx_max);
// The weights' image, if a tensor was loaded since the last upload (one blocking copy).
int taco_upload_if_dirty(wrnn_taco_handle *h);
