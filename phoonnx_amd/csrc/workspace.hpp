// workspace.hpp — the device workspaces of a VITS run, each stated once as the walk that carves it (slab.hpp).
// Host-side C++17: model.hpp and the carver only, so the plans can be exercised without a device.
//
// A walk takes the model and the sizes of a request - never an option of one call: vits_reserve(B, T, F) sizes the slabs
// by the same walks and must cover whatever call comes later, so a buffer only some calls use (per-utterance settings,
// seeds, forced durations, the prior noise, the chunk lengths) is carved for all of them.  Branches follow the model.
// Every walk's size is non-decreasing in each of its sizes: a reservation for the largest request covers the smaller ones.
#pragma once
#include <cstdint>
#include <cstdlib>
#include <vector>

#include "delivery.hpp"
#include "fit.hpp"
#include "limit.hpp"
#include "loudness.hpp"
#include "model.hpp"
#include "resample.hpp"
#include "shape.hpp"
#include "slab.hpp"
#include "stream_shape.hpp"
#include "warp.hpp"

namespace vitsmi {

// attention on the 16-bit matrix pipe as f16x3 products (attention16.hip.hpp): head widths of 32 / 64 / 96, q | k | v given as
// operand planes too (the q|k|v conv's planar epilogue writes them).  VITSMI_ATT16=0 keeps the fp32-MFMA kernel (A/B timing).
inline bool attention16_ok(int dk, int window) {
    static const bool off = [] { const char *e = std::getenv("VITSMI_ATT16"); return e && e[0] == '0'; }();
    return !off && dk % 32 == 0 && dk <= 96 && window <= 4;
}

// operand planes are 16-bit cells carved in floats: n fp32 elements as three plane slots + the whole-cell pad
constexpr size_t kPlanePad = 64;
inline size_t plane_floats(size_t n) { return n + n / 2 + kPlanePad; }
inline uint16_t *take_planes(Carver &cv, size_t nfloats) { return reinterpret_cast<uint16_t *>(cv.take<float>(nfloats)); }

// ---- token domain (vits_handle::tok): encoder + duration predictor + durations, B utterances of T tokens
struct TokenBufs {
    int *len, *cum;
    int64_t *ylen64;
    float *x, *att, *xe, *qkv, *ffh, *stats, *logw;
    float *wceil;     // [w_ceil B*T | y_len B | fit results, B records at the most]: one block, read back with one copy
    float *rows;      // per-utterance settings [B][3]
    uint64_t *seeds;  // per-utterance noise seeds [B]
    int64_t *ctl;     // forced durations (int64 [B][T]) or, in the same buffer, per-token rates (float [B][T])
    float *fit_w;     // a fitted run's weights [B][T] (tap "w")
    int64_t *fit_in;  // a fitted run's [target int64 B | group int32 B | mode int32 B], sent as one copy
    uint16_t *x_pl, *att_pl, *ff_pl, *qkv_pl;  // Model::enc_sx: operand planes of x, attn out, ffn hidden and q | k | v
    float *dp_cond;                            // Model::gin
    int pr_rows;  // spline parameters per position: 3 * bins - 1 (29 for the reference's 10 bins, up to 47)
    float *hb, *y, *y2, *cond, *h2, *pr, *z;   // stochastic duration predictor (h2: also the plain one's)
    float *xi, *h1;                            // plain duration predictor (xi: x + cond(g), Model::gin)
};

inline TokenBufs carve_tokens(Carver &cv, const Model &m, int B, int T) {
    TokenBufs t{};
    const size_t nBT = (size_t)B * T, nHT = nBT * m.H;
    t.len = cv.take<int>(B);
    t.ylen64 = cv.take<int64_t>(B);
    t.cum = cv.take<int>(nBT);
    t.x = cv.take<float>(nHT);
    t.att = cv.take<float>(nHT);
    t.xe = cv.take<float>(nHT);  // the embedded ids keep their own buffer (tap "emb"); layer 0 reads it and writes x
    t.qkv = cv.take<float>(3 * nHT);
    t.ffh = cv.take<float>(nBT * m.FF);
    t.stats = cv.take<float>(nBT * 2 * m.C);
    t.logw = cv.take<float>(nBT);
    t.wceil = cv.take<float>(fit_block_floats(nBT, B, B));
    t.rows = cv.take<float>((size_t)B * 3);
    t.seeds = cv.take<uint64_t>(B);
    t.ctl = cv.take<int64_t>(nBT);
    t.fit_w = cv.take<float>(nBT);
    t.fit_in = cv.take<int64_t>((size_t)B * 2);
    if (m.enc_sx) {
        t.x_pl = take_planes(cv, plane_floats(nHT));
        t.att_pl = take_planes(cv, plane_floats(nHT));
        t.ff_pl = take_planes(cv, plane_floats(nBT * m.FF));
        if (attention16_ok(m.dk, m.window)) t.qkv_pl = take_planes(cv, nHT * 9 / 2 + kPlanePad);
    }
    if (m.gin) t.dp_cond = cv.take<float>((size_t)B * m.dp_cond_rows);
    if (m.use_sdp) {
        const size_t n = nBT * m.dp_pre.Cout;
        t.pr_rows = 32;
        for (const auto &cf : m.cf) t.pr_rows = cf.proj.Cout > t.pr_rows ? cf.proj.Cout : t.pr_rows;
        t.hb = cv.take<float>(n);
        t.y = cv.take<float>(n);
        t.y2 = cv.take<float>(n);
        t.cond = cv.take<float>(n);
        t.h2 = cv.take<float>(n);
        t.pr = cv.take<float>(nBT * t.pr_rows);
        t.z = cv.take<float>(nBT * 2);
    } else {
        if (m.gin) t.xi = cv.take<float>(nHT);
        t.h1 = cv.take<float>(nBT * m.dpp_F);
        t.h2 = cv.take<float>(nBT * m.dpp_F);
    }
    return t;
}

// ---- frame domain (vits_handle::frm): [flow | vocoder input] then the generator

// the inverse coupling flow over B utterances of F frames (F a multiple of 4)
struct FlowBufs {
    float *zp, *z;
    float *g;  // the prior noise of a run that draws it from the flat stream
    float *hx, *skip, *acts, *a2;
    uint16_t *hx_pl, *x0_pl, *skip_pl;  // planes of hx (sx in-layers), of a coupling's x0 and of its skip sum (sx pre / post)
    std::vector<float *> gc;            // Model::gin: a coupling's speaker conditioning [B][2 * flow_H * n_wn]
    float *dec_cond;                    // Model::gin: the generator's [B][C0]
};

inline FlowBufs carve_flow(Carver &cv, const Model &m, int B, int F) {
    FlowBufs f{};
    const size_t nCF = (size_t)B * m.C * F, nHF = (size_t)B * m.flow_H * F;
    f.zp = cv.take<float>(nCF);
    f.z = cv.take<float>(nCF);
    f.g = cv.take<float>(nCF);
    f.hx = cv.take<float>(nHF);
    f.skip = cv.take<float>(nHF);
    f.acts = cv.take<float>(nHF);
    f.a2 = cv.take<float>(nHF * 2);
    f.hx_pl = take_planes(cv, nHF * 2);
    f.x0_pl = take_planes(cv, nCF);
    f.skip_pl = take_planes(cv, nHF * 2);
    if (m.gin) {
        for (const auto &cd : m.flow) f.gc.push_back(cv.take<float>((size_t)B * 2 * m.flow_H * cd.n_wn));
        f.dec_cond = cv.take<float>((size_t)B * m.C0);
    }
    return f;
}

// what a vocoder-only call puts in front of the generator: z [B][C][F] from the host, and the speaker bias
struct VocoderIn {
    float *z;
    int64_t *sid;     // Model::gin
    float *dec_cond;  // Model::gin
};

inline VocoderIn carve_vocoder_in(Carver &cv, const Model &m, int B, int F) {
    VocoderIn v{};
    v.z = cv.take<float>((size_t)B * m.C * F);
    if (m.gin) {
        v.sid = cv.take<int64_t>(B);
        v.dec_cond = cv.take<float>((size_t)B * m.C0);
    }
    return v;
}

// the generator's region: floats of its largest tensor when it renders F frames
inline size_t gen_region_floats(const Model &m, int B, int F) {
    size_t mx = (size_t)B * (m.C0 > m.C ? m.C0 : m.C) * ((F + 3) & ~3);
    int64_t t = F;
    for (auto &st : m.ups) {
        t *= st.u;
        size_t n = (size_t)B * st.C * t;
        mx = n > mx ? n : mx;
    }
    return mx;
}

// frames the generator renders at a time when F are asked for: everything, or (chunk_frames > 0) one chunk with its context
inline int gen_frames(const Model &m, int F, int chunk_frames) {
    const int n = chunk_frames + 2 * m.gen_rf_frames;
    return chunk_frames > 0 && n < F ? n : F;
}

// The three generator walkers' buffers; what a walker does not use stays null.
struct GenBufs {
    int *yl;  // the frame counts of the chunk being rendered
    // split-operand walkers: plane tensors (R elements each as three 16-bit slots; they double as fp32 raw buffers where a
    // stage uses the raw format), the fp32 multi-receptive-field sum, and (raw-stream walker) the fp32 residual stream
    uint16_t *stage_in[2], *y_pl, *raa[2], *tmp_pl;
    float *xs_raw, *y_raw, *ra[2];
    float *reg[10];  // f32 engine: ten fp32 regions; the waveform is the last
    float *out;      // the waveform [B][F * hop]
};

inline GenBufs carve_generator(Carver &cv, const Model &m, int B, int F) {
    GenBufs g{};
    const size_t R = gen_region_floats(m, B, F);
    g.yl = cv.take<int>(B);
    if (!m.gen_sx) {
        for (auto &r : g.reg) r = cv.take<float>(R);
        g.out = g.reg[9];
        return g;
    }
    for (uint16_t **p : {&g.stage_in[0], &g.stage_in[1], &g.y_pl, &g.raa[0], &g.raa[1], &g.tmp_pl}) *p = take_planes(cv, plane_floats(R));
    if (!m.gen_planes) {
        g.y_raw = cv.take<float>(R);
        g.ra[0] = cv.take<float>(R);
        g.ra[1] = cv.take<float>(R);
    }
    g.xs_raw = cv.take<float>(R);
    g.out = cv.take<float>((size_t)B * F * m.hop);
    return g;
}

// The whole frame-domain slab of a request: B utterances, F frames in front of the generator (a multiple of 4 for the
// flow), the generator rendering Fgen at a time (gen_frames).  `flow`: a synthesis run; false: a vocoder-only call.
struct FrameBufs {
    FlowBufs flow;
    VocoderIn voc;
    size_t gen_at;  // mark in front of the generator's part: each chunk of a chunked run carves it again
    GenBufs gen;
};

inline FrameBufs carve_frames(Carver &cv, const Model &m, int B, int F, int Fgen, bool flow) {
    FrameBufs f{};
    if (flow) f.flow = carve_flow(cv, m, B, F);
    else f.voc = carve_vocoder_in(cv, m, B, F);
    f.gen_at = cv.mark();
    f.gen = carve_generator(cv, m, B, Fgen);
    return f;
}

// ---- staging slab (vits_handle::io): the host inputs of a call, or - between runs - the 16-bit waveform

// ids | lens | sid contiguous (they arrive in one copy), then the injected noises: noise_dp [B][2][Tdp] and noise_z [B][C][Fz]
// (Tdp, Fz: the tokens / frames per row of the noise a caller passes - sizes of the request like B and T; 0 without one)
struct InputBufs {
    int64_t *ids, *lens, *sid;
    float *noise_dp, *noise_z;
};

inline InputBufs carve_inputs(Carver &cv, const Model &m, int B, int T, int Tdp, int64_t Fz) {
    InputBufs i{};
    i.ids = cv.take<int64_t>((size_t)B * T + 2 * (size_t)B);
    if (i.ids) {
        i.lens = i.ids + (size_t)B * T;
        i.sid = i.lens + B;
    }
    i.noise_dp = cv.take<float>((size_t)B * 2 * Tdp);
    i.noise_z = cv.take<float>((size_t)B * m.C * Fz);
    return i;
}

// vits_last_pcm16: the int16 waveform [B][S] and the per-utterance peaks
struct PcmBufs {
    int16_t *pcm;
    unsigned *peak;
};

inline PcmBufs carve_pcm16(Carver &cv, int B, int S) {
    PcmBufs p{};
    p.pcm = cv.take<int16_t>((size_t)B * S);
    p.peak = cv.take<unsigned>(B);
    return p;
}

// vits_deliver: the packed, encoded audio of the segments (whole 16-byte cells), the segment table and the peak slots (one
// per row, one per stream).  Every row is in at most one segment, so the request bounds all three: at most 4 * B * S bytes
// of audio (F32), B segments, 2 * B slots - whatever plan and encoding a call brings.
struct DeliveryBufs {
    unsigned char *packed;
    DeliverySeg *segs;
    unsigned *peak;
};

inline DeliveryBufs carve_delivery(Carver &cv, int B, int S) {
    DeliveryBufs d{};
    d.packed = cv.take<unsigned char>((size_t)B * S * 4 + 16);
    d.segs = cv.take<DeliverySeg>(B);
    d.peak = cv.take<unsigned>(2 * (size_t)B);
    return d;
}

// vits_deliver_trimmed on top of the delivery's buffers (a walk of its own, behind them): the scan's bounds - {first, last}
// active index per segment, preset to {INT_MAX, -1} - and the untrimmed rows' peaks the relative thresholds read.  At most
// B segments.
struct TrimBufs {
    int32_t *bounds;
    unsigned *peak_all;
};

inline TrimBufs carve_trim(Carver &cv, int B) {
    TrimBufs t{};
    t.bounds = cv.take<int32_t>(2 * (size_t)B);
    t.peak_all = cv.take<unsigned>(B);
    return t;
}

// vits_deliver_leveled on top of both (a walk of its own, behind carve_trim's): the table of the levelled segments, the
// states behind and in front of every chunk, the chunks' partial sums, and ONE result buffer the host fetches in one copy -
// the segments' sample peaks [B] and behind them the sub-block energies.  Sized by the request: every row is in at most one
// segment, a row of n <= S samples has at most S / kLoudChunk + 1 chunks and, at the smallest admitted rate's hop, at most
// S / kLoudMinHop sub-blocks.
struct LevelBufs {
    LoudSeg *segs;
    LoudState *fin, *init;
    float *part;
    unsigned *result;  // [B] peaks (float bits), then the energies (float)
    float *e() const { return reinterpret_cast<float *>(result) + n_peaks; }
    size_t n_peaks, n_chunks, n_subs;
};

inline LevelBufs carve_level(Carver &cv, int B, int S) {
    LevelBufs l{};
    l.n_peaks = (size_t)B;
    l.n_chunks = (size_t)B * ((size_t)S / kLoudChunk + 1);
    l.n_subs = (size_t)B * ((size_t)S / kLoudMinHop);
    l.segs = cv.take<LoudSeg>(B);
    l.fin = cv.take<LoudState>(l.n_chunks);
    l.init = cv.take<LoudState>(l.n_chunks);
    l.part = cv.take<float>(l.n_chunks * kLoudParts);
    l.result = cv.take<unsigned>(l.n_peaks + l.n_subs);
    return l;
}

// vits_deliver_shaped on top of the three (a walk of its own, behind carve_level's - or behind carve_trim's where nothing is
// levelled): the shape records parallel to the segment table, and the segments' knots (shape.hpp: a segment's points and
// one more).  At most B segments; n_knots is the call's, shape_knot_count.
struct ShapeBufs {
    ShapeSeg *segs;
    ShapeKnot *knots;
};

inline ShapeBufs carve_shape(Carver &cv, int B, int64_t n_knots) {
    ShapeBufs s{};
    s.segs = cv.take<ShapeSeg>(B);
    s.knots = cv.take<ShapeKnot>((size_t)n_knots);
    return s;
}

// vits_deliver_limited on top of the four (a walk of its own, carved last): the limit records parallel to the segment table,
// and the gain of every packed element - fp32 [B * S], since every row is in at most one segment.
struct LimitBufs {
    LimitSeg *segs;
    float *gain;
};

inline LimitBufs carve_limit(Carver &cv, int B, int S) {
    LimitBufs l{};
    l.segs = cv.take<LimitSeg>(B);
    l.gain = cv.take<float>((size_t)B * S);
    return l;
}

// With an output rate set (vits_set_output_rate), the staging slab holds the run's RESULT once its inputs are consumed:
// the resampled fp32 waveform [B][S_out] (a chunked run: the output samples of one chunk, never more than S_out per
// row), the rows' valid input and output sample counts, the two generations of the chunked path's carry [B][K] (the
// last K input samples of every row; one is read while the other is written), and behind them vits_last_pcm16's buffers
// and then vits_deliver's for that waveform - one walk, so that converting or delivering it never moves it.  With a rate per
// row (vits_set_output_rates) it is the same walk: S_out is the longest row's count, K the largest among the rows' plans.
struct ResampleBufs {
    float *out;
    int *n_in, *n_out;
    float *carry[2];
    PcmBufs pcm;
    DeliveryBufs dlv;
};

inline ResampleBufs carve_resample(Carver &cv, int B, int S_out, int K) {
    ResampleBufs r{};
    r.out = cv.take<float>((size_t)B * S_out);
    r.n_in = cv.take<int>(B);
    r.n_out = cv.take<int>(B);
    for (auto &c : r.carry) c = cv.take<float>((size_t)B * K);
    r.pcm = carve_pcm16(cv, B, S_out);
    r.dlv = carve_delivery(cv, B, S_out);
    return r;
}

// A warped run (vits_run_async_warped) leaves its result in the staging slab the same way: carve_resample's walk for rows of
// S_w samples without a carry (K = 0) - so vits_last_pcm16 and vits_deliver*, which carve it again to find their buffers
// behind the waveform, find them where they are - with the rows' output counts in n_out, and behind it the plan the one
// launch reads: the segment records and the rows' records, one block, uploaded in one copy.  A delivery's own buffers may
// reuse the plan block: the launch that read it precedes them on the stream.  Used by warp_run alone; vits_reserve does
// not count it.
struct WarpBufs {
    ResampleBufs front;
    vits_warp_seg *segs;
    void *rows;  // [B] records of row_bytes each: WarpRow, or - a folded launch ("pitch at an output rate") - WarpRateRow
    size_t plan_bytes;  // segs | rows
};

inline WarpBufs carve_warp(Carver &cv, int B, int S_w, int64_t n_segs, size_t row_bytes = sizeof(WarpRow)) {
    WarpBufs w{};
    w.front = carve_resample(cv, B, S_w, 0);
    w.plan_bytes = (size_t)n_segs * sizeof(vits_warp_seg) + (size_t)B * row_bytes;
    char *p = cv.take<char>(w.plan_bytes);
    if (p) {
        w.segs = reinterpret_cast<vits_warp_seg *>(p);
        w.rows = p + (size_t)n_segs * sizeof(vits_warp_seg);
    }
    return w;
}

// A streamed run with pitch (vits_run_chunked_glided, "streamed pitch") has these in front of carve_stream's in the same walk:
// the history - the run's native waveform [B][row_in], appended to piece by piece: rows at different speeds need different
// amounts of past input, without `compensate` unboundedly much -, the output of one windowed launch [B][n_cap], the rows'
// output counts (what the pack stage masks by) and the plan block of carve_warp.  vits_reserve does not count it.
struct WarpStreamBufs {
    float *hist;
    int64_t hist_pitch;
    float *out;
    int *n_out;
    vits_warp_seg *segs;
    void *rows;  // [B] records of row_bytes each, as WarpBufs::rows
    size_t plan_bytes;  // segs | rows
};

inline WarpStreamBufs carve_warp_stream(Carver &cv, int B, int64_t row_in, int64_t n_cap, int64_t n_segs, size_t row_bytes = sizeof(WarpRow)) {
    WarpStreamBufs w{};
    w.hist_pitch = row_in;
    w.hist = cv.take<float>((size_t)B * row_in);
    w.out = cv.take<float>((size_t)B * n_cap);
    w.n_out = cv.take<int>(B);
    w.plan_bytes = (size_t)n_segs * sizeof(vits_warp_seg) + (size_t)B * row_bytes;
    char *p = cv.take<char>(w.plan_bytes);
    if (p) {
        w.segs = reinterpret_cast<vits_warp_seg *>(p);
        w.rows = p + (size_t)n_segs * sizeof(vits_warp_seg);
    }
    return w;
}

// The buffers of ONE delivery call, whichever entry it came through, and the one walk that carves them: the delivery's own
// (carved here, or - `front` - those a carve_resample in the same walk has just carved behind the resampled waveform), then
// what the call's stages need, in this order: the trim slots of a call that scans (every one but vits_deliver), the level
// buffers where a segment is levelled, the shape tables where one is shaped - or limited: the limiter reads every segment's
// shape record, a one-knot envelope of gain 1 where it has none -, the limiter's buffers last.  vits_reserve walks it with
// everything on.
struct DeliveryNeeds {
    bool scan, levelled, shaped;
    int64_t n_knots;       // shape_knot_count; a limited call without shapes: one per segment
    bool limited = false;  // (implies shaped)
};

struct DeliveryCallBufs {
    DeliveryBufs dlv;
    TrimBufs trim;
    LevelBufs level;
    ShapeBufs shape;
    LimitBufs limit;
};

inline DeliveryCallBufs carve_delivery_call(Carver &cv, int B, int S, const DeliveryNeeds &need, const DeliveryBufs *front = nullptr) {
    DeliveryCallBufs c{};
    c.dlv = front ? *front : carve_delivery(cv, B, S);
    if (!need.scan) return c;
    c.trim = carve_trim(cv, B);
    if (need.levelled) c.level = carve_level(cv, B, S);
    if (need.shaped) c.shape = carve_shape(cv, B, need.n_knots);
    if (need.limited) c.limit = carve_limit(cv, B, S);
    return c;
}

// An encoded stream (vits_run_chunked_enc): one device buffer [chunk bytes | running peaks | format table].  `cap` bytes hold
// the largest chunk in the widest encoding - B rows of n_max samples as F32 at a 16-byte row pitch - whatever encoding and
// chunk_frames a call brings; the running peaks [B] (padded to whole 16-byte cells) sit right behind at a 16-byte-aligned
// offset and never move, and a chunk's [B][pitch] bytes END at them (at()), so one copy of B * pitch + 4 * B bytes carries a
// chunk and its peaks.  Behind the peaks: {ref_peak, volume} per row, uploaded with the peaks' zeros in one copy per run.
// A trimmed stream (vits_run_chunked_enc_trimmed) has the rows' starts [B] (int32, padded like the peaks) between the peaks and
// the format table: the one copy then carries bytes, peaks and starts, B * pitch + 4 * (peak_floats(B) + B) bytes.
// Carved by carve_stream (below) and nowhere else.
struct StreamPackBufs {
    unsigned char *buf;
    size_t cap;
    unsigned *peak_run;
    float *fmt;
    int32_t *start = nullptr;  // a trimmed stream's; right behind the peaks
    static size_t pitch(int width, int64_t n) { return (size_t)(((int64_t)width * n + 15) & ~(int64_t)15); }
    static size_t peak_floats(int B) { return ((size_t)B + 3) & ~size_t(3); }
    unsigned char *at(int B, size_t row_pitch) const { return buf + cap - (size_t)B * row_pitch; }  // row_pitch <= pitch(4, n_max)
};

inline StreamPackBufs carve_stream_pack(Carver &cv, int B, int64_t n_max, bool trimmed = false) {
    StreamPackBufs s{};
    s.cap = (size_t)B * StreamPackBufs::pitch(4, n_max);
    const size_t starts = trimmed ? StreamPackBufs::peak_floats(B) : 0;
    s.buf = cv.take<unsigned char>(s.cap + (StreamPackBufs::peak_floats(B) + starts + 2 * (size_t)B) * sizeof(float));
    if (s.buf) {
        s.peak_run = reinterpret_cast<unsigned *>(s.buf + s.cap);
        if (trimmed) s.start = reinterpret_cast<int32_t *>(s.peak_run + StreamPackBufs::peak_floats(B));
        s.fmt = reinterpret_cast<float *>(s.peak_run) + StreamPackBufs::peak_floats(B) + starts;
    }
    return s;
}

// A shaped, limited encoded stream (vits_run_chunked_enc_shaped) has this behind carve_stream_pack in the same walk (carve_stream):
// the rows' records and the knots of their envelopes, and the two generations of the limiter's carry - the last 2 L raw samples
// of every row, one read while the other is written.  The chunk buffer's L extra samples per row - the last chunk delivers L
// more than it renders - are carve_stream_pack's: the caller hands it n_max + L.
struct StreamShapeBufs {
    StreamShapeRow *rows;
    ShapeKnot *knots;
    float *carry[2];
    StreamOnsetRow *onsets = nullptr;  // a trimmed stream's: what the scan reads (stream_trim.hip.hpp), carved last
};

inline StreamShapeBufs carve_stream_shape(Carver &cv, int B, int L, int64_t n_knots, bool trimmed = false) {
    StreamShapeBufs s{};
    s.rows = cv.take<StreamShapeRow>(B);
    s.knots = cv.take<ShapeKnot>((size_t)n_knots);
    for (auto &c : s.carry) c = cv.take<float>((size_t)B * 2 * L);
    if (trimmed) s.onsets = cv.take<StreamOnsetRow>(B);
    return s;
}

// ---- a streamed run (vitsmi.hip, render_chunks; its stages: stream_run.hip.hpp): the sizes of its pieces - host arithmetic, so
// that a CPU program can walk every schedule - and the ONE walk of the staging slab.  A chunk renders input samples [f0 * hop, f1 * hop);
// at an output rate it completes the outputs whose K inputs all exist; a look-ahead of L delivers what lies L behind that (stream_emit_range).

// output samples one chunk of `chunk` frames (of F) can complete at the output rate, at most S_out
inline int64_t resample_emit_cap(const ResamplePlan &rp, int chunk, int F, int hop, int64_t S_out) {
    const int64_t cap = rp.count((int64_t)(chunk < F ? chunk : F) * hop + rp.K / 2) + 2;
    return cap < S_out ? cap : S_out;
}

// the output samples complete once the input in front of position `end` exists (the last piece: all S_out)
inline int64_t resample_emit_end(const ResamplePlan &rp, int64_t end, bool is_last, int64_t S_out) {
    const int64_t done = rp.complete(end);
    return is_last || done > S_out ? S_out : done;
}

// samples per row of the largest piece a run delivers: what a chunk renders (at a rate: completes) + the look-ahead L, at most the row
inline int64_t stream_n_max(const ResamplePlan &rp, int chunk, int F, int hop, int L, int64_t total) {
    const int64_t piece = rp.on() ? resample_emit_cap(rp, chunk, F, hop, total) : (int64_t)(chunk < F ? chunk : F) * hop;
    return piece + L < total ? piece + L : total;
}

// bytes of one pinned ring slot: B rows of the largest piece as fp32 (width 0: a float sink) or encoded, the running peaks behind -
// and behind them a trimmed stream's starts
inline size_t stream_ring_bytes(int B, int64_t n_max, int width, bool trimmed = false) {
    if (!width) return (size_t)B * n_max * sizeof(float);
    return (size_t)B * StreamPackBufs::pitch(width, n_max) + StreamPackBufs::peak_floats(B) * (trimmed ? 2 : 1) * sizeof(float);
}

// What a streamed run takes from the staging slab (from its base: the run's inputs are consumed), in this order: at an output
// rate (K > 0: the resampler's) carve_resample's buffers for rows of `row` output samples - the chunk the stream packs lives
// there -, an encoded sink's chunk buffer for pieces of n_max samples, a shaped one's tables and carries.  The rest stays zero.
// trimmed (implies shaped: a trimmed stream runs the shaped kernels): the rows' starts and the scan's records on top.
struct StreamBufs {
    ResampleBufs rs;
    StreamPackBufs sp;
    StreamShapeBufs ss;
};

inline StreamBufs carve_stream(Carver &cv, int B, int64_t row, int64_t n_max, int K, bool enc, bool shaped, int L, int64_t n_knots,
                               bool trimmed = false) {
    StreamBufs s{};
    if (K > 0) s.rs = carve_resample(cv, B, (int)row, K);
    if (enc) s.sp = carve_stream_pack(cv, B, n_max, trimmed);
    if (enc && shaped) s.ss = carve_stream_shape(cv, B, L, n_knots, trimmed);
    return s;
}

}  // namespace vitsmi
