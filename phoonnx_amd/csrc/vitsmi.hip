// vitsmi.hip — host side of libvitsmi.so: handle, workspace, the VITS pipeline as a sequence of
// kernel launches on one HIP stream, and the C ABI declared in include/vitsmi.h.
//
// Pipeline = SynthesizerTrn.infer (phoonnx_train/vits/models.py:681-722):
//   text encoder -> (stochastic) duration predictor -> length regulator -> inverse coupling flow
//   -> HiFi-GAN generator.  The only host synchronisation inside a run is the readback of the frame
//   counts (data-dependent output length).
#include <climits>
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdarg>
#include <chrono>
#include <cstdio>
#include <cstring>
#include <mutex>
#include <string>
#include <vector>

#include "../../include/vitsmi.h"
#include "conv_geom.hpp"
#include "conv_sx_engine.hip.hpp"
#include "conv_sx_pair.hip.hpp"
#include "conv_sx_pair16.hip.hpp"
#include "attention16.hip.hpp"
#include "conv_sx_small.hip.hpp"
#include "delivery.hip.hpp"
#include "delivery_run.hip.hpp"
#include "fit.hip.hpp"
#include "shape.hip.hpp"
#include "kernels.hip.hpp"
#include "loudness.hip.hpp"
#include "model.hpp"
#include "resample.hip.hpp"
#include "stream_pack.hip.hpp"
#include "stream_run.hip.hpp"
#include "stream_shape.hip.hpp"
#include "test_dev.hip.hpp"
#include "warp.hip.hpp"
#include "workspace.hpp"

using namespace vitsmi;

namespace {

thread_local std::string g_open_error;

// One device allocation, carved anew by every run: its size comes from a dry walk of the run's plan (workspace.hpp), its
// buffers from the same walk over a Carver on [base, base + cap).
struct Slab {
    char *base = nullptr;
    size_t cap = 0;
};

// Pinned host buffer handed out by vits_run()/vits_run_vocoder() and returned by vits_free_output():
// one per handle, reused across calls (hipHostMalloc costs more than a whole B=1 run).
struct PinnedPool {
    char *base = nullptr;
    size_t cap = 0;
    bool busy = false;
};

}  // namespace

struct vits_handle {
    Model model;
    int device = -1;
    bool host_only = false;
    hipStream_t stream = nullptr;
    float *arena_dev = nullptr;
    bool arena_owned = false;
    Slab tok, frm;  // token-domain and frame-domain workspaces
    Slab io;        // device staging of vits_run()'s host inputs
    PinnedPool pin;
    std::mutex mu;
    std::string err;
    // last-run state (for taps / outputs)
    int B = 0, T = 0, F = 0, S = 0;
    int Fpitch = 0;  // row pitch of the frame-domain flow tensors (F rounded up to 4)
    float *d_emb = nullptr, *d_x = nullptr, *d_mp = nullptr, *d_logs = nullptr, *d_logw = nullptr, *d_wceil = nullptr;
    float *d_zp = nullptr, *d_z = nullptr, *d_out = nullptr;
    int *d_len = nullptr, *d_ylen = nullptr, *d_cum = nullptr;
    int64_t *d_ylen64 = nullptr;
    std::vector<int> h_ylen;
    char *h_in_pin = nullptr;      // pinned staging of a call's ids | lens | sid: one host-to-device copy instead of three
    size_t h_in_pin_bytes = 0;     // staged pageable ones
    // vits_last_durations: the host copy of w_ceil [B][T].  It sits in front of y_len in the token slab, so the one mid-run
    // readback fetches [w_ceil | y_len] in ONE copy - the same number of copies and synchronisations as the frame counts
    // alone.  h_dur_B == 0: no token run to report (never ran, a workspace grew, a vocoder-only run).
    std::vector<float> h_dur;
    float *h_rb_pin = nullptr;     // pinned landing buffer of that readback: [B * T floats | B ints] (a pageable destination
    size_t h_rb_pin_n = 0;         // makes the copy a staged, synchronous one: the stream then waits for the host twice)
    int h_dur_B = 0, h_dur_T = 0;
    bool last_forced = false;      // the last run took its durations from the caller: no logw to tap
    // vits_last_fit / tap "w": the per-group results of the last run when it was fitted (they ride in the readback block
    // behind y_len), and its weights [B][T] in the token slab
    std::vector<FitResult> h_fit;
    float *d_fit_w = nullptr;
    // stats
    int timing = 0;  // vits_set_timing: 0 off, 1 stage marks + events around every conv launch, 2 stage marks only
    vits_stats stats{};
    std::vector<std::pair<hipEvent_t, hipEvent_t>> conv_events;
    std::vector<char> conv_event_sx;  // 1: that launch went through the split-exact engine
    std::vector<vits_launch_record> conv_recs;  // what each timed launch was (vits_launch_records)
    size_t conv_events_used = 0;
    hipEvent_t ev[6] = {nullptr, nullptr, nullptr, nullptr, nullptr, nullptr};
    int cur_stage = 0;  // 0 enc, 1 dp, 2 flow, 3 dec
    uint64_t run_counter = 0;
    // Padded batches (B > 1, unequal frame counts).  The reference graph does not mask its generator (models.py:348-368, 720):
    // it renders every utterance to the longest one's length and the samples behind an utterance's end are the generator's
    // response to zeros.  tails_reference = false (default; VITSMI_TAILS=reference or vits_set_tails(h, 1) for the other):
    // those samples are NOT rendered - every generator launch ends utterance b's tensors gen_rf_frames behind y_len[b]
    // (SxRagged), so each valid sample is bit-identical to the padded rendering - and the output holds zeros there.
    bool tails_reference = false;
    int gen_nprod = 2;  // generator arithmetic (VITSMI_GEN_PRECISION): 2 = two fp16 planes / three products (default), 6 = six
                        // exact bf16 plane products, 1 = one fp16 plane / one product with fp16 activations (config 4)
    // f16 range guard: every launch that splits values into fp16 planes publishes the largest magnitude it saw into its
    // own 64 slots of d_range; range_reduce_kernel folds them at the end of a run into d_range_res = {max, min over
    // launches of the per-launch peak, launches tracked}, copied to the pinned h_range (read after the next sync).
    unsigned *d_range = nullptr;
    float *d_range_res = nullptr;
    float *h_range = nullptr;
    int range_launch = 0;
    int range_used = -1;          // slots groups the last run wrote (-1: unknown, clear all)
    int h_range_launches = 0;     // launches behind the values in h_range
    bool range_pending = false;   // h_range holds the result of a run that has not been checked yet
    bool range_failed = false;    // the last run saturated (sticky until the next run starts)
    // chunked rendering: two pinned host buffers the finished chunks are copied into, with their completion events
    char *ring[2] = {nullptr, nullptr};
    size_t ring_cap = 0;
    hipEvent_t ring_ev[2] = {nullptr, nullptr};
    // Output rate (vits_set_output_rate): the plan and, on a device handle, its table.  rs.plan.on() == false: every path is
    // the native one.  A run with a rate leaves its resampled waveform in the staging slab: d_out / S then describe THAT
    // buffer, out_resampled says so, d_nout holds the rows' output sample counts (vits_last_pcm16's valid lengths) and
    // rs_run_K the K its walk was carved with.
    ResampleDev rs;
    bool out_resampled = false;
    int *d_nout = nullptr;
    int rs_run_K = 0;
    int64_t rs_run_L = 1, rs_run_M = 1;  // ... and the ratio its sample counts follow (vits_deliver's valid lengths)
    // A rate per row (vits_set_output_rates): the rows' rates as given, the distinct plans among them - at most
    // VITS_MAX_ROW_RATES, each with its table on a device handle - and on the device one plan record per row.  rows.on()
    // excludes rs.plan.on().  A run under it whose rows are not all native goes through the same buffers as one at a handle
    // rate (out_resampled, d_nout, rs_run_K: the largest K); run_rates / run_L / run_M describe the rows of that run, and of
    // an all-native one, and are empty after every other run.
    struct RowRates {
        int fi = 0;
        std::vector<int32_t> fo;         // [n_rows]; 0 or fi: native
        std::vector<int> plan_of;        // [n_rows] index into plans; -1: native
        std::vector<ResampleDev> plans;  // keyed by (fi, fo)
        ResampleRowPlan *d_recs = nullptr;
        int lds = 0;                     // the largest staged span among the plans
        bool on() const { return !fo.empty(); }
    } rows;
    std::vector<int32_t> run_rates;
    std::vector<int64_t> run_L, run_M;
    bool last_vocoder = false;          // the last run was vocoder-only: every row has F frames, h_ylen is not its
    // Intonation (vits_run_async_warped): the prototype table on the device (made by the first warped run), the pinned buffer
    // a run's plan is uploaded from, and what the last warped run left for the host: its rows' output counts N_b - empty
    // after every other run - and k per token [B][T].  The warped waveform lives in the staging slab as a resampled one does
    // (out_resampled, d_nout, rs_run_K = 0).
    float *warp_G = nullptr;
    char *warp_pin = nullptr;
    size_t warp_pin_cap = 0;
    std::vector<int64_t> warp_counts, warp_spans;
    int warp_T = 0;
    // vits_set_pitch_at_rate: a pitched run with an output rate set folds the rate into the warp's step ("pitch at an output
    // rate").  Off - the default -, such a run is refused as it always was.
    bool pitch_at_rate = false;
};

// chunked rendering (vits_run_chunked / vits_run_vocoder_chunked): where the audio goes
struct ChunkSink {
    int chunk_frames;
    vits_chunk_fn fn;
    void *user;
    // the encoded form (vits_run_chunked_enc): fmt != nullptr, validated; the chunks go to efn, not to fn
    const vits_stream_format *fmt = nullptr;
    vits_enc_chunk_fn efn = nullptr;
    // ... shaped (vits_run_chunked_enc_shaped): validated, nullable
    const vits_stream_shaping *shaping = nullptr;
    // ... trimmed (vits_run_chunked_enc_trimmed): validated, nullable; its chunks go to tfn, with the rows' skips
    const vits_stream_onset *onsets = nullptr;
    vits_enc_chunk_trim_fn tfn = nullptr;
};

constexpr int kMaxRangeLaunches = 512;

namespace {

int fail(vits_handle *h, int code, const char *fmt, ...) {
    char buf[1024];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof buf, fmt, ap);
    va_end(ap);
    if (h) h->err = buf;
    else g_open_error = buf;
    return code;
}

// this launch's slots of the f16 range guard (nullptr when the arithmetic has no fp16 planes)
unsigned *range_slots(vits_handle *h, bool f16) {
    if (!f16 || !h->d_range) return nullptr;
    const int i = h->range_launch < kMaxRangeLaunches ? h->range_launch : kMaxRangeLaunches - 1;
    h->range_launch++;
    return h->d_range + (size_t)i * kSxPeakSlots * kSxPeakStride;
}

// one wave per launch: peak = max over its 64 slots; out[0] = max over launches, out[1] = min over the launches that
// recorded anything (both as float bit patterns, which order like unsigned integers for non-negative floats; preset
// to 0 / 0xffffffff by range_end)
__global__ void range_reduce_kernel(const unsigned *slots, unsigned *out) {
    unsigned b = slots[((size_t)blockIdx.x * kSxPeakSlots + threadIdx.x) * kSxPeakStride];
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) b = max(b, (unsigned)__shfl_xor((int)b, o, 64));
    if (threadIdx.x == 0 && b) {  // (an all-zero tensor - e.g. fully masked rows - says nothing about range)
        atomicMax(out, b);
        atomicMin(out + 1, b);
    }
}

void range_begin(vits_handle *h) {
    h->range_launch = 0;
    // (only the slots the previous run used need clearing)
    if (h->d_range)
        hipMemsetAsync(h->d_range, 0, (size_t)(h->range_used > 0 ? h->range_used : kMaxRangeLaunches) * kSxPeakSlots *
                                          kSxPeakStride * sizeof(unsigned), h->stream);
}

// fold the slots and start the 12-byte copy to the host; evaluated by range_check() after the next synchronisation
void range_end(vits_handle *h) {
    if (!h->d_range) return;
    const int n = h->range_launch < kMaxRangeLaunches ? h->range_launch : kMaxRangeLaunches;
    h->range_used = n;
    unsigned *res = reinterpret_cast<unsigned *>(h->d_range_res);
    hipMemsetAsync(res, 0, 4, h->stream);
    hipMemsetAsync(res + 1, 0xff, 4, h->stream);
    if (n > 0) range_reduce_kernel<<<n, kSxPeakSlots, 0, h->stream>>>(h->d_range, res);
    hipMemcpyAsync(h->h_range, h->d_range_res, 2 * sizeof(float), hipMemcpyDeviceToHost, h->stream);
    h->h_range_launches = n;
    h->range_pending = true;
}

// after a synchronisation: did the last run leave the fp16 planes' range?
int range_check(vits_handle *h) {
    if (!h->range_pending) return 0;
    h->range_pending = false;
    unsigned bits[2];
    std::memcpy(bits, h->h_range, sizeof bits);
    float pmax, pmin;
    std::memcpy(&pmax, &bits[0], 4);
    if (bits[1] == 0xffffffffu) pmin = 0.f;  // nothing recorded
    else std::memcpy(&pmin, &bits[1], 4);
    h->stats.f16_peak_max = pmax;
    h->stats.f16_peak_min = pmin;
    h->stats.f16_tracked = h->h_range_launches;
    h->stats.f16_saturated = !(pmax <= kF16Max) ? 1 : 0;
    h->range_failed = h->stats.f16_saturated != 0;
    if (h->stats.f16_saturated)
        return fail(h, VITS_E_RANGE,
                    "an activation of magnitude %g (or a non-finite value) left the range of the generator's fp16 operand "
                    "planes (65504): the f16x3 arithmetic would clamp it.  Open the voice with gen_precision \"bf16x6\" "
                    "(VITSMI_GEN_PRECISION=bf16x6), whose bf16 planes have the fp32 range",
                    (double)h->stats.f16_peak_max);
    return 0;
}

#define HIPCHECK(h, expr)                                                                       \
    do {                                                                                        \
        hipError_t _e = (expr);                                                                 \
        if (_e != hipSuccess)                                                                   \
            return fail(h, VITS_E_DEVICE, "%s failed: %s (%s:%d)", #expr, hipGetErrorString(_e), \
                        __FILE__, __LINE__);                                                    \
    } while (0)

// (slack: a request that needs more than any before it gets a quarter on top - the frame count of the SAME batch moves by
// +-7 % with the noise of a pass - so that growth stops after the first requests; vits_reserve asks for exactly what its
// caller said)
// A workspace that is about to be freed takes the last run's results with it: everything vits_fetch_output /
// vits_last_pcm16 / vits_tap (and a caller of vits_run_device / vits_run_async still holding out->data) would read lives
// in tok or frm.  Those pointers are dropped here, so the next such call fails with "no completed run" instead of reading
// freed device memory (a run that grows a slab sets them again itself, behind the growth).
void forget_results_in(vits_handle *h, const Slab &s) {
    if (&s == &h->tok) {
        h->d_emb = h->d_x = h->d_mp = h->d_logs = h->d_logw = h->d_wceil = h->d_fit_w = nullptr;
        h->d_len = h->d_ylen = h->d_cum = nullptr;
        h->d_ylen64 = nullptr;
        h->h_dur_B = h->h_dur_T = 0;
    } else if (&s == &h->frm) {
        h->d_zp = h->d_z = nullptr;
        if (!h->out_resampled) h->d_out = nullptr;
    } else if (&s == &h->io && h->out_resampled) {  // (with an output rate set the waveform lives in the staging slab)
        h->d_out = nullptr;
        h->d_nout = nullptr;
        h->out_resampled = false;
    }
}

// a run that begins is not (yet) one with a rate per row
void forget_row_run(vits_handle *h) {
    h->warp_counts.clear();  // (nor a warped one)
    h->warp_spans.clear();
    h->run_rates.clear();
    h->run_L.clear();
    h->run_M.clear();
}

// With a rate per row set (vits_set_output_rates), what an entry must meet before anything is staged or enqueued - the
// previous run stays readable: the chunked entries and the device-pointer entries (`uncovered`: the entry's name) are not
// covered, and a run has exactly the rows that were named.
int row_rates_admit(vits_handle *h, int B, const char *uncovered) {
    if (!h->rows.on()) return 0;
    if (uncovered) return fail(h, VITS_E_ARG, "%s is not covered with per-row output rates", uncovered);
    if (B != (int)h->rows.fo.size())
        return fail(h, VITS_E_ARG, "a run of B = %d rows, vits_set_output_rates named %d rows", B, (int)h->rows.fo.size());
    return 0;
}

int slab_reserve(vits_handle *h, Slab &s, size_t bytes, bool slack = true) {
    if (bytes <= s.cap) return 0;
    if (s.base) {
        HIPCHECK(h, hipStreamSynchronize(h->stream));
        forget_results_in(h, s);
        HIPCHECK(h, hipFree(s.base));
        s.base = nullptr;
        s.cap = 0;
    }
    size_t want = bytes + (slack ? bytes / 4 : 0) + (1 << 20);
    static const bool trace = std::getenv("VITSMI_TRACE_ALLOC") != nullptr;
    const auto t0 = std::chrono::steady_clock::now();
    hipError_t e = hipMalloc((void **)&s.base, want);
    if (trace)
        fprintf(stderr, "vitsmi: handle %p slab %p grows to %.1f MB (hipMalloc %.1f ms)\n", (void *)h, (void *)&s, want / 1e6,
                std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count());
    if (e != hipSuccess) {
        (void)hipGetLastError();  // (the error is reported HERE: the next launch check must not find it)
        return fail(h, VITS_E_NOMEM, "hipMalloc(%zu) failed: %s", want, hipGetErrorString(e));
    }
    s.cap = want;
    return 0;
}

// Reserve what `walk` measures dry, then run it over the slab.  The check behind the real walk cannot fire while both are
// one function of the same arguments; it is there so that a later mistake is an error here, before any launch, and not a
// kernel writing past the allocation.
template <class Walk>
int slab_carve(vits_handle *h, Slab &s, const char *name, Walk &&walk) {
    if (int rc = slab_reserve(h, s, carved_bytes(walk))) return rc;
    Carver cv(s.base, s.cap);
    walk(cv);
    if (!cv.fits()) return fail(h, VITS_E_NOMEM, "%s workspace: its walk carved %zu bytes of the %zu reserved", name, cv.used, cv.cap);
    return 0;
}

struct Ctx {
    vits_handle *h;
    const Model &m;
    hipStream_t st;
    const float *A;  // device arena
    int B;
    hipError_t err = hipSuccess;
    // ragged generator (run_generator*): device frame counts + margin, the frame count F the launches' T are multiples of, and
    // the share of B * F frames that lies inside the utterances' (margin-extended) ends - what the FLOP / byte accounting of a
    // generator launch is scaled by (host copy of the frame counts: h_len)
    SxRagged rag{nullptr, 0, 0};
    int rag_F = 0;
    double rag_frac = 1.0;
    const int *h_len = nullptr;
    const float *P(int64_t off) const { return off >= 0 ? A + off : nullptr; }
    // the SxRagged of a generator launch whose input tensors have T columns per utterance
    SxRagged rag_at(int T) const {
        if (!rag.len || rag_F <= 0 || T % rag_F) return SxRagged{nullptr, 0, 0};
        return SxRagged{rag.len, rag.add, T / rag_F};
    }
    double work_frac() const { return rag.len ? rag_frac : 1.0; }
    // the flow's convs on a padded batch (conv_sx): frames behind y_len[b] are neither read nor written (device frame counts;
    // the share of B * F frames inside the utterances, for the accounting)
    const int *flow_len = nullptr;
    double flow_frac = 1.0;
    void note(hipError_t e) {
        if (err == hipSuccess && e != hipSuccess) err = e;
    }
};

// algorithmic FLOPs / layer-granular bytes of one conv launch, per pipeline stage
void conv_account(Ctx &c, const ConvDesc &d, int T) {
    vits_handle *h = c.h;
    // (ragged generator launches: only the columns inside the utterances' ends are worked on)
    const double wf = c.h->cur_stage == 2 && c.flow_len ? c.flow_frac : c.work_frac();
    double fl = 2.0 * d.macs_per_t * (double)T * c.B * wf;
    double by = (d.h1 ? 2.0 : 4.0) * c.B * ((double)d.Cin * T + (double)d.Cout * T) * wf;  // (stored dtype: SURVEY 8d)
    h->stats.conv_flops += fl;
    h->stats.conv_bytes += by;
    h->stats.conv_launches++;
    h->stats.total_launches++;
    switch (h->cur_stage) {
        case 0: h->stats.enc_flops += fl; break;
        case 1: h->stats.dp_flops += fl; break;
        case 2: h->stats.flow_flops += fl; break;
        default:
            h->stats.dec_flops += fl;
            h->stats.dec_bytes += by;
            break;
    }
}

// with timing enabled: record the start event of the next conv launch (the caller records the end event)
bool conv_event_begin(Ctx &c) {
    vits_handle *h = c.h;
    if (h->timing != 1) return false;
    if (h->conv_events_used == h->conv_events.size()) {
        hipEvent_t e0, e1;
        hipEventCreate(&e0);
        hipEventCreate(&e1);
        h->conv_events.push_back({e0, e1});
    }
    if (h->conv_event_sx.size() < h->conv_events.size()) h->conv_event_sx.resize(h->conv_events.size(), 0);
    if (h->conv_recs.size() < h->conv_events.size()) h->conv_recs.resize(h->conv_events.size());
    h->conv_event_sx[h->conv_events_used] = 0;
    g_launch_name[0] = 0;
    hipEventRecord(h->conv_events[h->conv_events_used].first, c.st);
    return true;
}

// ... and its end event, with what the launch was: the instantiation the launcher picked (g_launch_name), algorithmic
// FLOPs and layer-granular bytes
void conv_event_end(Ctx &c, bool sx, double flops, double bytes, const ConvDesc &d, int T) {
    vits_handle *h = c.h;
    const size_t i = h->conv_events_used++;
    h->conv_event_sx[i] = sx ? 1 : 0;
    vits_launch_record &r = h->conv_recs[i];
    std::snprintf(r.kernel, sizeof r.kernel, "%s", g_launch_name);
    r.flops = flops;
    r.bytes = bytes;
    r.stage = h->cur_stage;
    r.ms = 0.f;
    r.cin = d.Cin;
    r.cout = d.Cout;
    r.k = d.K;
    r.dil = d.dil;
    r.t = T;
    hipEventRecord(h->conv_events[i].second, c.st);
}

// What a launch's arguments take from the conv's descriptor, for conv() / conv_sx() and the kernel test hooks alike (A: the
// arena the descriptor's offsets count from; zeros: its zero page).  Everything else is the caller's.
ConvArgs conv_args(const ConvDesc &d, const float *A, const float *zeros) {
    ConvArgs a{};
    a.wp = A + d.w_off;
    a.bias = d.b_off >= 0 ? A + d.b_off : nullptr;
    a.zeros = zeros;
    a.Cin = d.Cin;
    a.Cout = d.Cout;
    a.K = d.K;
    a.dil = d.dil;
    a.padL = d.padL;
    a.CK = d.CK;
    a.nchunks = d.nchunks;
    a.ups = d.ups;
    a.div = 1.f;  // (EPI_DIV's operand: neutral until a caller sets one)
    return a;
}

// ... of the split-operand engine, for an input of T columns: the batch strides are those of whole tensors in the engine's
// layouts (conv_sx() below)
SxArgs sx_args(const ConvDesc &d, const float *A, const float *zeros, int T) {
    SxArgs a{};
    const int Cr = d.Cout / d.ups;
    a.x_bstride = (int64_t)3 * (d.Cin / 8) * T;
    a.T = T;
    a.wp = reinterpret_cast<const u32x4 *>(A + d.w_off);
    a.bias = d.b_off >= 0 ? A + d.b_off : nullptr;
    a.raw_bstride = (int64_t)Cr * T * d.ups;
    a.pl_bstride = 3 * a.raw_bstride;
    a.zeros = zeros;
    a.Cin = d.Cin;
    a.Cout = d.Cout;
    a.Cr = Cr;
    a.K = d.K;
    a.dil = d.dil;
    a.padL = d.padL;
    a.nchunks = d.nchunks;
    a.ups = d.ups;
    a.div = 1.f;
    a.wscale = d.wscale;
    a.s16 = d.s16 ? 1 : 0;
    static const bool zt_off = std::getenv("VITSMI_NO_ZERO_TAP_SKIP") != nullptr;  // A/B timing
    a.zt_p = zt_off ? -1 : d.zt_p;
    return a;
}

// Launch one conv through the engine; accounts algorithmic FLOPs/bytes per stage.
struct ConvOpt {                      // the optional arguments of conv(), set by name
    const int *len = nullptr;         // [B] valid lengths (the mask flags, EPI_WN, EPI_COUPLING)
    const float *res = nullptr;       // EPI_RES operand and its batch stride
    int64_t res_bstride = 0;
    const float *bias_b = nullptr;    // per-utterance bias [B][bias_b_stride]
    int bias_b_stride = 0;
    float slope = 0.1f;               // PRO_LRELU
    float div = 1.f;                  // EPI_DIV
    float oslope = 1.f;               // leaky_relu slope of the value stored in out (1 = none) ...
    float *out2 = nullptr;            // ... and in the optional second output
    float oslope2 = 1.f;
    int x_cstride = 0;                // floats between the channels of x (0 = T)
    int out_cstride = 0;              // ... of out / out2 / res (0 = T * ups)
    int wn_split = 0;                 // EPI_WN: first skip row
    uint16_t *out_pl = nullptr;       // fp16 operand planes of the rows [0, pl_rows) of `out` for a following sx conv
    int pl_rows = 0;
};

void conv(Ctx &c, const ConvDesc &d, const float *x, int64_t x_bstride, int T, float *out, int64_t out_bstride,
          int flags, const ConvOpt &o = {}) {
    ConvArgs a = conv_args(d, c.A, c.P(c.m.zeros_off));
    a.x = x;
    a.x_bstride = x_bstride;
    a.x_cstride = o.x_cstride;
    a.T = T;
    a.len = o.len;
    a.bias_b = o.bias_b;
    a.bias_b_stride = o.bias_b_stride;
    a.out = out;
    a.out_bstride = out_bstride;
    a.out_cstride = o.out_cstride;
    a.out2 = o.out2;
    a.res = o.res;
    a.res_bstride = o.res_bstride;
    a.flags = flags;
    a.slope = o.slope;
    a.div = o.div;
    a.oslope = o.oslope;
    a.oslope2 = o.oslope2;
    a.wn_split = o.wn_split;
    a.out_pl = o.out_pl;
    a.pl_rows = o.pl_rows;
    a.peak = o.out_pl ? range_slots(c.h, true) : nullptr;
    const bool ev = conv_event_begin(c);
    c.note(launch_conv(a, d.cfg, c.B, c.st));
    if (ev) conv_event_end(c, false, 2.0 * d.macs_per_t * (double)T * c.B, 4.0 * c.B * ((double)d.Cin * T + (double)d.Cout * T), d, T);
    conv_account(c, d, T);
}

// One conv through the split-operand engine (conv_sx_engine.hip.hpp; 16-bit planes: fp16 x 2 by default, bf16 x 3).  Tensors are whole utterance
// batches in the engine's layouts: input planes [B][3][Cin/8][T][8], outputs raw [B][Cr/8][T*u][8] and/or
// planes [B][3][Cr/8][T*u][8]; `res` has the raw layout of the output.
// `x` is the plane tensor, or (d.rawin) the fp32 raw tensor, to which the kernel applies leaky_relu(islope).
struct SxOpt {                        // the optional arguments of conv_sx(), set by name
    const float *res = nullptr;       // EPI_RES operand: fp32, the layout of out_raw ...
    const uint16_t *res_pl = nullptr;  // ... or (d.h1, the residual-plane instantiations) the plane tensor that holds
    float res_slope = 1.f;             //     leaky_relu(residual, res_slope)
    const float *bias_b = nullptr;    // per-utterance bias [B][bias_b_stride]
    int bias_b_stride = 0;
    float div = 1.f;                  // EPI_DIV
    float oslope = 1.f, oslope2 = 1.f;  // leaky_relu slope of the value stored in out_raw / split into out_pl (1 = none)
    float islope = 1.f;               // d.rawin: leaky_relu slope applied to x on the way in
    // SX_WN_RMW (the planar epilogue):
    const int *len = nullptr;
    float *out_raw2 = nullptr;
    int row_split = 0, pl_rows = 0;   // first row that goes to out_raw2; planes of the first pl_rows rows only
    bool pl_of2 = false;              // planes of out_raw2's rows instead of out_raw's
    int64_t planar_bstride = 0;       // batch stride of out_raw / res (0: row_split * T)
};

// largest launch (in workgroups of the short-launch kernel) that conv_sx() hands to conv_sx_small_kernel; process-wide,
// VITSMI_SX_SMALL_MAX at start-up, vits_test_set_sx_small_max() for A/B tests
std::atomic<long long> &sx_small_max() {
    static std::atomic<long long> v{[] { const char *e = std::getenv("VITSMI_SX_SMALL_MAX"); return e ? std::atoll(e) : 1536ll; }()};
    return v;
}

void conv_sx(Ctx &c, const ConvDesc &d, const void *x, int T, float *out_raw, uint16_t *out_pl, int flags,
             const SxOpt &o = {}) {
    SxArgs a = sx_args(d, c.A, c.P(c.m.zeros_off), T);
    const int64_t Tout = (int64_t)T * d.ups;
    if (d.rawin) a.xr = static_cast<const float *>(x);
    else a.xp = static_cast<const u32x4 *>(x);
    a.islope = o.islope;
    a.bias_b = o.bias_b;
    a.bias_b_stride = o.bias_b_stride;
    a.out_raw = out_raw;
    a.out_pl = out_pl;
    if (flags & SX_GATE) {  // half the rows: planar acts [H][T] / planes of the H acts
        a.raw_bstride = (int64_t)(a.Cr / 2) * Tout;
        a.pl_bstride = 3 * a.raw_bstride;
    }
    a.len = o.len;
    a.out_raw2 = o.out_raw2;
    a.row_split = o.row_split;
    a.pl_rows = o.pl_rows;
    if (flags & SX_WN_RMW) a.pl_bstride = (int64_t)3 * o.pl_rows * Tout;
    a.pl_of2 = o.pl_of2 ? 1 : 0;
    a.planar_bstride = o.planar_bstride;
    a.res = o.res;
    a.res_pl = o.res_pl;
    a.res_unslope = 1.f / o.res_slope;
    a.flags = flags;
    a.div = o.div;
    a.oslope = o.oslope;
    a.oslope2 = o.oslope2;
    vits_handle *h = c.h;
    if (h->cur_stage == 3) a.rag = c.rag_at(T);
    // the flow's tensors are masked by y_len (modules.py:447-466: every conv's input is x * mask, every result * mask): a
    // padded batch's frames behind an utterance's end are zeros the reference computes and this engine neither reads nor
    // writes (run_frames: Ctx::flow_len, when every launch of the flow is one of these)
    else if (h->cur_stage == 2 && c.flow_len) a.rag = SxRagged{c.flow_len, 0, 1};
    a.peak = range_slots(h, (d.f16 || d.h1) && (d.rawin || out_pl));  // launches that turn values into fp16 planes
    const bool ev = conv_event_begin(c);
    // Short grids (a single utterance, a streaming chunk): the 128-row packing is read by the 64- or 32-row kernel -
    // 2-4x the workgroups, each with half / a quarter of the reduction work per step.  Same arithmetic.
    static const bool tall_only = std::getenv("VITSMI_SX_NO_SHORT_TILES") != nullptr;  // A/B timing only
    int run_cfg = d.cfg;
    if (d.cfg == 0 && !d.rawin && !tall_only) {
        const long long wgs0 = (long long)((T + 255) / 256) * c.B * (d.Cout / 128);
        if (wgs0 <= 128) run_cfg = 2;
        else if (wgs0 <= 256) run_cfg = 1;
        // token- / frame-domain convs with the planar epilogue (short reductions, bound by their prologue / epilogue
        // latencies): 64 x 128 tiles put 4-7x the workgroups on the chip (res_skip 51 -> 42 us, FFN conv_1 43 -> 36 us)
        if (d.s16 && (flags & SX_WN_RMW) && wgs0 > 128 && wgs0 <= 1024) run_cfg = 3;
    }
    // 64-row layers on the 16x16x32 loop: 128-column tiles where the grid of 256-column ones fills the chip badly (the
    // flow's WN in-layers at batch 32: 768 workgroups on 512 slots = two rounds of which the second is half empty, and 24 %
    // padding columns; as 1344 half-size workgroups on 768 slots: the time of one full round).  Same arithmetic.
    static const bool no_narrow = std::getenv("VITSMI_SX_NO_NARROW_TILES") != nullptr;  // A/B timing only
    if (d.cfg == 1 && d.s16 && !d.rawin && !no_narrow) {
        const long long mt = d.Cout / 64;
        const long long w256 = ((long long)((T + 255) / 256) * c.B + 7) / 8 * 8 * mt, w128 = ((long long)((T + 127) / 128) * c.B + 7) / 8 * 8 * mt;
        const long long r256 = (w256 + 511) / 512 * 2, r128 = (w128 + 767) / 768;  // rounds, in units of a 128-column tile
        if (r128 < r256) run_cfg = 3;
    }
    {
        // (experiments only: VITSMI_SX_FORCE_CFG=<stage><cfg>, e.g. 22 = the flow's plane-input convs on the 32-row tile)
        static const int force = [] { const char *e = std::getenv("VITSMI_SX_FORCE_CFG"); return e ? std::atoi(e) : -1; }();
        if (force >= 0 && d.s16 && !d.rawin && h->cur_stage == force / 10 && (!(flags & SX_GATE) || force % 10 == 1 || force % 10 == 3) &&
            sx_tile_m(force % 10) <= sx_tile_m(d.cfg) && d.Cout % sx_tile_m(force % 10) == 0)
            run_cfg = force % 10;
    }
    // Short launches of the token / frame domain (one utterance, a streaming chunk): the reduction-splitting kernel of
    // conv_sx_small.hip.hpp.  VITSMI_SX_SMALL_MAX = largest launch in workgroups that takes it (0: never; A/B timing).
    const long long small_max = sx_small_max().load(std::memory_order_relaxed);
    const int nprod = d.h1 ? 1 : (d.f16 ? 2 : 6);
    // (generator convs - neither planar nor gated - stay on the engine whatever the launch size: a chunked rendering
    // (vits_run_chunked) must equal the unchunked one bit for bit, so a conv's kernel must not depend on how many frames a launch
    // covers.  VITSMI_SX_SMALL_GEN=1 lifts that for single-shot latency: 1.31 -> 1.27 ms on `medium`, 3.34 -> 3.24 on `high`.)
    static const bool small_gen = [] { const char *e = std::getenv("VITSMI_SX_SMALL_GEN"); return e && e[0] == '1'; }();
    const bool small_kind = (a.flags & (SX_WN_RMW | SX_GATE)) != 0 || small_gen;
    if (small_max > 0 && small_kind && conv_sx_small_ok(a, d.rawin, nprod) && conv_sx_small_wgs(a, c.B) <= small_max)
        c.note(launch_conv_sx_small(a, c.B, d.cfg, c.st));
    else
        c.note(launch_conv_sx(a, run_cfg, c.B, c.st, d.rawin, nprod, d.cfg));
    // layer-granular bytes in the STORED dtype ("bf16 storage halves these"): 2 bytes per element in the
    // single-plane mode, 4 otherwise
    const double ebytes = d.h1 ? 2.0 : 4.0;
    const double wf = !a.rag.len ? 1.0 : (h->cur_stage == 2 ? c.flow_frac : c.rag_frac);
    const double fl = 2.0 * d.macs_per_t * (double)T * c.B * wf, by = ebytes * c.B * ((double)d.Cin * T + (double)d.Cout * T) * wf;
    if (ev) conv_event_end(c, true, fl, by, d, T);
    conv_account(c, d, T);
    h->stats.sx_flops += fl;
    h->stats.sx_bytes += by;
    h->stats.sx_launches++;
}

constexpr int kAttMaxHeadWidth = 128;  // attention_relpos_kernel<4, KH>: ceil(dk / 32) <= 4
// a3: relative-position attention core, one launch (kernels.hip.hpp).  Two key halves per workgroup unless
// VITSMI_ATT_NOSPLIT is set (A/B timing only); kh = 1 / 2 (the kernel-level test hook) names the key halves itself.
template <int DKB, int KH>
void launch_attention_t(hipStream_t st, dim3 grid, const float *qkv, float *att, const float *rel_k, const float *rel_v,
                        const int *len, int H, int T, int dk, int window, uint16_t *planes, unsigned *peak) {
    if (g_launch_name_on) snprintf(g_launch_name, sizeof g_launch_name, "attention_relpos_kernel<%d, %d>", DKB, KH);
    attention_relpos_kernel<DKB, KH><<<grid, 256 * KH, 0, st>>>(qkv, att, rel_k, rel_v, len, H, T, dk, window, planes, peak);
}
void launch_attention(hipStream_t st, int B, int T, int n_heads, int dk, int window, const float *qkv, float *att,
                      const float *rel_k, const float *rel_v, const int *len, int H, uint16_t *planes = nullptr,
                      unsigned *peak = nullptr, int kh = 0) {
    static const bool nosplit = std::getenv("VITSMI_ATT_NOSPLIT") != nullptr;
    const bool one_half = kh ? kh == 1 : nosplit;
    dim3 ag((T + 127) / 128, n_heads, B);
    const int dkb = (dk + 31) / 32;
#define VITSMI_ATT(DKB)                                                                                             \
    do {                                                                                                            \
        if (one_half) launch_attention_t<DKB, 1>(st, ag, qkv, att, rel_k, rel_v, len, H, T, dk, window, planes, peak); \
        else launch_attention_t<DKB, 2>(st, ag, qkv, att, rel_k, rel_v, len, H, T, dk, window, planes, peak);          \
    } while (0)
    switch (dkb) {
        case 1: VITSMI_ATT(1); break;
        case 2: VITSMI_ATT(2); break;
        case 3: VITSMI_ATT(3); break;
        default: VITSMI_ATT(4); break;
    }
#undef VITSMI_ATT
}

// ... on the 16-bit matrix pipe as f16x3 products (attention16.hip.hpp) where attention16_ok (workspace.hpp)
template <int DKS, int NS, int QT>
hipError_t launch_attention16_t(hipStream_t st, const Att16Args &a) {
    constexpr int lds = NS * 4 * (DKS * 2) * 1024 + 9 * DKS * 32 * 4 + 16 + 64 * QT * kAtt16RelPitch * 4;
    static std::atomic<uint64_t> done{0};
    if (lds > 64 * 1024)
        if (hipError_t e = sx_allow_big_lds(reinterpret_cast<const void *>(&attention_relpos16_kernel<DKS, NS, QT>), done)) return e;
    const int ntile = (a.T + 64 * QT - 1) / (64 * QT), npair = a.nh * a.B;
    if (g_launch_name_on) snprintf(g_launch_name, sizeof g_launch_name, "attention_relpos16_kernel<%d, %d, %d>", DKS, NS, QT);
    attention_relpos16_kernel<DKS, NS, QT><<<dim3(((npair + 7) / 8) * 8 * ntile), 256, lds, st>>>(a);
    return hipSuccess;
}
// stages / query tiles per wave: two stages, 64 queries per workgroup; VITSMI_ATT16_NS / VITSMI_ATT16_QT override (A/B timing),
// and ns_arg / qt_arg (the kernel-level test hook; 0 = not given) override those
hipError_t launch_attention16(hipStream_t st, int B, int T, int n_heads, int dk, int window, const uint16_t *qkv_pl, float *att,
                              uint16_t *att_pl, const float *rel_k, const float *rel_v, const int *len, int H, unsigned *peak,
                              unsigned long long *prof = nullptr, int ns_arg = 0, int qt_arg = 0) {
    static const int env_ns = [] { const char *e = std::getenv("VITSMI_ATT16_NS"); return e ? std::atoi(e) : 0; }();
    static const int env_qt = [] { const char *e = std::getenv("VITSMI_ATT16_QT"); return e ? std::atoi(e) : 0; }();
    Att16Args a{};
    a.qkv_pl = qkv_pl;
    a.out = att;
    a.out_pl = att_pl;
    a.relk = rel_k;
    a.relv = rel_v;
    a.len = len;
    a.Hc = H;
    a.T = T;
    a.dk = dk;
    a.win = window;
    a.nh = n_heads;
    a.B = B;
    a.peak = att_pl ? peak : nullptr;
    a.prof = prof;
    const int ns = ns_arg ? ns_arg : (env_ns ? env_ns : 2), qt = qt_arg ? qt_arg : (env_qt ? env_qt : 1);  // (measured: 2, 3 and 4 stages time alike)
    if (dk == 32) return launch_attention16_t<1, 3, 1>(st, a);
    if (dk == 64) return launch_attention16_t<2, 3, 1>(st, a);
    if (qt == 2) return ns >= 3 ? launch_attention16_t<3, 3, 2>(st, a) : launch_attention16_t<3, 2, 2>(st, a);
    if (ns >= 4) return launch_attention16_t<3, 4, 1>(st, a);
    return ns == 3 ? launch_attention16_t<3, 3, 1>(st, a) : launch_attention16_t<3, 2, 1>(st, a);
}

// The token-to-frame and frame-to-sample kernels (kernels.hip.hpp), one launch each.  The pipeline and the kernel-level test
// hooks (vits_test_durations ...) both launch through these, so each kernel's grid is stated once.
void launch_durations(hipStream_t st, int B, int T, const float *logw, const int *len, float length_scale, const float *rows,
                      const float *token_rate, float *w_ceil, int *cum, int *y_len) {
    duration_kernel<<<B, 256, 0, st>>>(logw, len, length_scale, rows, token_rate, w_ceil, cum, y_len, T);
}

// fitted durations (fit.hip.hpp): w from logw by duration_kernel's own expression ...
void launch_fit_weights(hipStream_t st, int B, int T, const float *logw, const int *len, float length_scale, const float *rows,
                        const float *token_rate, float *w) {
    fit_weight_kernel<<<dim3((T + 255) / 256, B), 256, 0, st>>>(logw, len, length_scale, rows, token_rate, w, T);
}

// ... and the fit itself, one workgroup per group, over the rows the groups name
void launch_fit_durations(hipStream_t st, int B, int T, int G, const float *w, const int *len, const int *group, const int64_t *target,
                          const int *mode, float *w_ceil, int *cum, int *y_len, FitResult *res) {
    fit_duration_kernel<<<G, 256, 0, st>>>(w, len, group, target, mode, B, T, w_ceil, cum, y_len, res);
}

void launch_forced_durations(hipStream_t st, int B, int T, const int64_t *dur, const int *len, float *w_ceil, int *cum, int *y_len) {
    forced_duration_kernel<<<B, 256, 0, st>>>(dur, len, w_ceil, cum, y_len, T);
}

// out [B][channels][T] = the utterances' own stream `stream` times column `col` of rows
void launch_fill_normal_rows(hipStream_t st, int B, int channels, int T, float *out, const uint64_t *seeds, uint32_t stream,
                             const float *rows, int col) {
    fill_normal_rows_kernel<<<dim3((unsigned)(((T + 3) / 4 + 63) / 64), channels, B), 64, 0, st>>>(out, T, seeds, stream, rows, col);
}

void launch_fill_normal(hipStream_t st, float *out, int64_t n, uint64_t seed, uint64_t stream_id) {
    fill_normal_kernel<<<(unsigned)((n / 4 + 256) / 256), 256, 0, st>>>(out, n, seed, stream_id);
}

void launch_expand_prior(hipStream_t st, int B, int C, int T, int F, const float *m_p, const float *logs_p, int64_t bstride,
                         const int *cum, const int *len, const int *y_len, const float *noise, int64_t noise_stride,
                         float noise_scale, const float *rows, const uint64_t *seeds, float *z_p, int Fnoise) {
    expand_prior_strided_kernel<<<dim3((F + 255) / 256, (C + 3) / 4, B), 64, 0, st>>>(m_p, logs_p, bstride, cum, len, y_len, noise,
                                                                                     noise_stride, noise_scale, rows, seeds, z_p, C,
                                                                                     T, F, Fnoise);
}

// the vocoder's tail on the planar layout (the f32 generator) ...
size_t post_conv_lds(int C, int K) { return ((size_t)C * (256 + K - 1) + (size_t)C * K) * sizeof(float); }
void launch_post_conv(hipStream_t st, int B, int C, int K, int T, const float *x, const float *w, float *out, float slope,
                      const int *vlen, int hop) {
    const size_t lds = post_conv_lds(C, K);
    post_conv_tanh_kernel<<<dim3((T + 255) / 256, B), 256, lds, st>>>(x, w, out, C, K, T, slope, vlen, hop);
}

// ... and on the fp32 raw layout [C/8][T][8] of the split-operand walkers (generic: the runtime tap count even for K = 7)
size_t post_conv_blocked_lds(int C, int K) { return (size_t)C * (256 + K - 1) * sizeof(float); }
void launch_post_conv_blocked(hipStream_t st, int B, int C, int K, int T, const float *x, const float *w, float *out, float slope,
                              const int *vlen, int hop, bool generic = false) {
    const size_t lds = post_conv_blocked_lds(C, K);
    if (K == 7 && !generic)
        post_conv_tanh_blocked_kernel<7><<<dim3((T + 255) / 256, B), 256, lds, st>>>(x, w, out, C, K, T, slope, vlen, hop);
    else
        post_conv_tanh_blocked_kernel<0><<<dim3((T + 255) / 256, B), 256, lds, st>>>(x, w, out, C, K, T, slope, vlen, hop);
}

// A token- / frame-domain conv on the split-operand engine with the planar epilogue (SX_WN_RMW): x_pl = fp16 operand planes
// of the input; out (may be nullptr when out_pl is given) = planar fp32 [B][Cout][T]; out_pl = operand planes of the output
// for the next conv; flags = EPI_RELU | EPI_MASK | EPI_ACC | EPI_RES; of the options o.len (the masks) and o.res (planar, the
// shape of out) are the caller's.
void conv_sx_planar(Ctx &c, const ConvDesc &d, const uint16_t *x_pl, int T, float *out, uint16_t *out_pl, int flags,
                    SxOpt o = {}) {
    o.row_split = d.Cout;
    o.pl_rows = out_pl ? d.Cout : 0;
    conv_sx(c, d, x_pl, T, out, out_pl, SX_WN_RMW | flags, o);
}

// planar fp32 [B][C][T] (masked by len when given) -> fp16 operand planes of the split-operand engine
void split_planes(Ctx &c, const float *x, uint16_t *pl, int C, int T, const int *len) {
    sx_split_planes_kernel<<<dim3((T + 255) / 256, C / 8, c.B), 256, 0, c.st>>>(x, (int64_t)C * T, T, len, pl, C, T, 1,
                                                                                range_slots(c.h, true));
    c.note(hipGetLastError());
    c.h->stats.total_launches++;
}

// What follows the launch of n dependent convs as ONE kernel (conv_sx_pair, conv_sx_pair16, conv_sx_mrf): the end event, whose
// record names the conv `rec`, and the counters - every member is accounted as a conv, the launches that did not happen
// are taken off again.  fl / by: algorithmic FLOPs and layer-granular bytes of the whole launch.
void fused_launch_end(Ctx &c, bool ev, const ConvDesc *const *members, int n, const ConvDesc &rec, int T, double fl, double by) {
    vits_stats &st = c.h->stats;
    if (ev) conv_event_end(c, true, fl, by, rec, T);
    for (int i = 0; i < n; i++) conv_account(c, *members[i], T);
    st.conv_launches -= n - 1;
    st.total_launches -= n - 1;
    st.sx_flops += fl;
    st.sx_bytes += by;
    st.sx_launches++;
}

// Two dependent convs of a ResBlock as ONE launch (conv_sx_pair.hip.hpp), raw-format stages only (x, out: fp32 raw
// [B][C/8][T][8]): a ResBlock1 step, out = c2(lrelu(c1(lrelu(x)))) + x, or (chain) two ResBlock2 steps,
// x1 = c1(lrelu(x)) + x, out = c2(lrelu(x1)) + x1; then [+ out] [/ div].
bool sx_pair_ok(const vits_handle *h, const ConvDesc &c1, const ConvDesc &c2) {
    static const bool off = std::getenv("VITSMI_SX_NO_PAIR") != nullptr;  // A/B timing only
    return !off && h->gen_nprod == 2 && c1.f16 && c2.f16 && c1.rawin && c2.rawin && c1.cfg == c2.cfg && c1.ups == 1 &&
           c2.ups == 1 && c1.Cin == c1.Cout && c2.Cin == c2.Cout && c1.Cin == c2.Cin && c2.padL * 2 == (c2.K - 1) * c2.dil &&
           sx_pair_supported(c1.Cin, c1.cfg, c1.K, c1.dil, c2.K, c2.dil);
}

// What a call site decides of a fused launch - the generator below and the kernel-level test hook (vits_test_conv_pair_sx_epi)
// fill SxPairArgs here and nowhere else; the tile geometry is launch_conv_sx_pair()'s.  A: the arena the convs were packed into,
// zeros: >= 1 KiB of zeros.
static SxPairArgs sx_pair_args(const ConvDesc &c1, const ConvDesc &c2, const float *A, const float *zeros, const float *x, int T, float *out,
                               int flags, float div, float slope, SxRagged rag, unsigned *peak) {
    SxPairArgs a{};
    const auto P = [A](int64_t off) { return off >= 0 ? A + off : nullptr; };
    a.xr = x;
    a.islope = slope;
    a.mslope = slope;
    a.T = T;
    a.wp1 = reinterpret_cast<const u32x4 *>(P(c1.w_off));
    a.wp2 = reinterpret_cast<const u32x4 *>(P(c2.w_off));
    a.bias1 = P(c1.b_off);
    a.bias2 = P(c2.b_off);
    a.wscale1 = c1.wscale;
    a.wscale2 = c2.wscale;
    a.out_raw = out;
    a.zeros = zeros;
    a.C = c1.Cin;
    a.K1 = c1.K;
    a.dil1 = c1.dil;
    a.pad1 = c1.padL;
    a.K2 = c2.K;
    a.dil2 = c2.dil;
    a.pad2 = c2.padL;
    a.flags = flags & (EPI_ACC | EPI_DIV);
    a.div = div;
    a.rag = rag;
    a.peak = peak;
    return a;
}

void conv_sx_pair(Ctx &c, const ConvDesc &c1, const ConvDesc &c2, const float *x, int T, float *out, int flags, float div,
                  float slope, bool chain = false) {
    vits_handle *h = c.h;
    SxPairArgs a = sx_pair_args(c1, c2, c.A, c.P(c.m.zeros_off), x, T, out, flags, div, slope, c.rag_at(T), range_slots(h, true));
#if SX_PAIR_PROF
    {
        // diagnostic build: one row of 8 counters per pair launch of a run, printed by the next launch_table / bench run
        static unsigned long long *rows = nullptr;
        static int idx = 0;
        if (!rows) {
            hipMalloc((void **)&rows, 64 * 8 * sizeof(unsigned long long));
            hipMemset(rows, 0, 64 * 8 * sizeof(unsigned long long));
        }
        if (h->stats.sx_launches == 0 || idx >= 64) idx = 0;
        a.prof = rows + (idx++ % 64) * 8;
        if (std::getenv("VITSMI_PAIR_PROF_DUMP") && idx == 1) {
            unsigned long long hrows[64 * 8];
            hipDeviceSynchronize();
            hipMemcpy(hrows, rows, sizeof hrows, hipMemcpyDeviceToHost);
            for (int r = 0; r < 64; r++)
                if (hrows[r * 8 + 7]) {
                    fprintf(stderr, "pairprof row %d wgs %llu:", r, hrows[r * 8 + 7]);
                    for (int i = 0; i < 7; i++) fprintf(stderr, " %.0f", (double)hrows[r * 8 + i] / (double)hrows[r * 8 + 7]);
                    fprintf(stderr, "\n");
                }
            hipMemset(rows, 0, sizeof hrows);
        }
    }
#endif
    const bool ev = conv_event_begin(c);
    c.note(launch_conv_sx_pair(a, c1.cfg, c.B, c.st, chain));
    const double wf = c.work_frac();
    const double fl = 2.0 * (c1.macs_per_t + c2.macs_per_t) * (double)T * c.B * wf;
    const double by = 4.0 * c.B * ((double)(c1.Cin + c1.Cout) * T + (double)(c2.Cin + c2.Cout) * T) * wf;
    const ConvDesc *const members[] = {&c1, &c2};
    fused_launch_end(c, ev, members, 2, c1, T, fl, by);
}

// Two dependent convs of a ResBlock on the 16x16x32 loop (conv_sx_pair16.hip.hpp): f16x3 (fp32 raw tensors; the convs'
// second weight copy, ConvDesc::w16_off) or the single-plane arithmetic (fp16 plane tensors).  VITSMI_PAIR16=0: off (A/B).
bool sx_pair16_ok(const vits_handle *h, const ConvDesc &c1, const ConvDesc &c2) {
    static const bool off = [] {
        const char *e = std::getenv("VITSMI_PAIR16");
        return (e && e[0] == '0') || std::getenv("VITSMI_SX_NO_PAIR") != nullptr;
    }();
    if (off || c1.Cin != c1.Cout || c2.Cin != c2.Cout || c1.Cin != c2.Cin || c1.ups != 1 || c2.ups != 1) return false;
    if (c1.padL * 2 != (c1.K - 1) * c1.dil || c2.padL * 2 != (c2.K - 1) * c2.dil) return false;
    const bool h1 = c1.h1 && c2.h1, f3 = c1.f16 && c2.f16 && c1.s16 && c2.s16 && !c1.rawin && !c2.rawin;
    if (!h1 && !f3) return false;
    if (c1.cfg != c2.cfg || c1.cfg != (c1.Cin == 64 ? 1 : 2)) return false;  // (weights packed for a tile of all C rows)
    (void)h;
    return sx_pair16_plan(c1.Cin, h1 ? 1 : 2, c1.K, c1.dil, c2.K, c2.dil, nullptr) != 0;
}

// What a call site decides of a fused launch - the generator below and the kernel-level test hook (vits_test_conv_pair16_epi)
// fill SxPair16Args here and nowhere else; the tile geometry is launch_conv_sx_pair16()'s.  A: the arena the convs were packed
// into, zeros: >= 1 KiB of zeros.
static SxPair16Args sx_pair16_args(const ConvDesc &c1, const ConvDesc &c2, const float *A, const float *zeros, const uint16_t *x, int T,
                                   float *out_raw, uint16_t *out_pl, int flags, float div, float slope, SxRagged rag, unsigned *peak) {
    SxPair16Args a{};
    const int C = c1.Cin;
    const auto P = [A](int64_t off) { return off >= 0 ? A + off : nullptr; };
    a.xpl = x;
    a.x_bstride = (int64_t)3 * C * T;
    a.islope = a.mslope = a.oslope = slope;
    a.T = T;
    a.wp1 = reinterpret_cast<const u32x4 *>(P(c1.w_off));
    a.wp2 = reinterpret_cast<const u32x4 *>(P(c2.w_off));
    a.bias1 = P(c1.b_off);
    a.bias2 = P(c2.b_off);
    a.wscale1 = c1.wscale;
    a.wscale2 = c2.wscale;
    a.out_raw = out_raw;
    a.raw_bstride = (int64_t)C * T;
    a.out_pl = out_pl;
    a.pl_bstride = (int64_t)3 * C * T;
    a.zeros = zeros;
    a.K1 = c1.K; a.dil1 = c1.dil; a.pad1 = c1.padL;
    a.K2 = c2.K; a.dil2 = c2.dil; a.pad2 = c2.padL;
    a.flags = flags;
    a.div = div;
    a.rag = rag;
    a.peak = peak;
    return a;
}

// x: the operand-plane tensor holding leaky_relu(x, slope) (two fp16 planes: f16x3; one: the single-plane arithmetic).
// out_raw: fp32 raw destination (flags & P16_HAS_RAW) and / or EPI_ACC operand; out_pl (flags & P16_HAS_PL): operand planes of
// leaky_relu(result, slope).
void conv_sx_pair16(Ctx &c, const ConvDesc &c1, const ConvDesc &c2, const uint16_t *x, int T, float *out_raw, uint16_t *out_pl, int flags,
                    float div, float slope, bool chain) {
    const bool h1 = c1.h1;
    const int C = c1.Cin;
    vits_handle *h = c.h;
    const SxPair16Args a = sx_pair16_args(c1, c2, c.A, c.P(c.m.zeros_off), x, T, out_raw, out_pl, flags, div, slope, c.rag_at(T),
                                          range_slots(h, true));
    const double ebytes = h1 ? 2.0 : 4.0;
    const bool ev = conv_event_begin(c);
    c.note(launch_conv_sx_pair16(a, C, h1 ? 1 : 2, c.B, c.st, chain));
    const double fl = 2.0 * (c1.macs_per_t + c2.macs_per_t) * (double)T * c.B * c.work_frac();
    const double by = ebytes * c.B * ((double)(c1.Cin + c1.Cout) * T + (double)(c2.Cin + c2.Cout) * T) * c.work_frac();
    const ConvDesc *const members[] = {&c1, &c2};
    fused_launch_end(c, ev, members, 2, c1, T, fl, by);
}

// The multi-receptive-field sum of a 32-channel ResBlock2 stage, xs = (rb_0(x) + .. + rb_{n-1}(x)) / n with every rb a
// two-step chain (models.py:356-363, modules.py:355-364), as ONE launch (conv_sx_pair_kernel<.., NCH = n>): can it?
bool sx_mrf_ok(const vits_handle *h, const UpStageDesc &stg) {
    // Opt-in (VITSMI_SX_MRF=1, read per run): measured on the default voice, the fused stage moves 4x fewer bytes and takes
    // the same time on one handle (2.39 vs 2.46 ms: the 32-row tiles are bound by their own dependent chains, not by HBM) and
    // loses 4-10 % of the step under the three-handle schedule (two long workgroups per CU instead of three short ones).
    const bool off = std::getenv("VITSMI_SX_MRF") == nullptr;
    const int n = (int)stg.rbs.size();
    if (off || n < 2 || n > 3) return false;
    int K1[3], d1[3], K2[3], d2[3];
    for (int j = 0; j < n; j++) {
        const auto &rb = stg.rbs[j];
        if (rb.type1 || rb.n != 2 || !sx_pair_ok(h, rb.c1[0], rb.c1[1]) || rb.c1[0].padL * 2 != (rb.c1[0].K - 1) * rb.c1[0].dil)
            return false;
        K1[j] = rb.c1[0].K;
        d1[j] = rb.c1[0].dil;
        K2[j] = rb.c1[1].K;
        d2[j] = rb.c1[1].dil;
    }
    return sx_mrf_geom(stg.rbs[0].c1[0].Cin, n, K1, d1, K2, d2, nullptr);
}

void conv_sx_mrf(Ctx &c, const UpStageDesc &stg, const float *x, int T, float *out, float slope) {
    const int n = (int)stg.rbs.size();
    SxPairArgs a{};
    a.xr = x;
    a.islope = slope;
    a.mslope = slope;
    a.T = T;
    a.out_raw = out;
    a.zeros = c.P(c.m.zeros_off);
    a.C = stg.rbs[0].c1[0].Cin;
    a.div = (float)n;
    a.nchain = n;
    double macs = 0, bytes = 0;
    const ConvDesc *members[6];  // (sx_mrf_ok: n <= 3)
    for (int j = 0; j < n; j++) {
        const ConvDesc &c1 = stg.rbs[j].c1[0], &c2 = stg.rbs[j].c1[1];
        members[2 * j] = &c1;
        members[2 * j + 1] = &c2;
        auto &ch = a.ch[j];
        ch.wp1 = reinterpret_cast<const u32x4 *>(c.P(c1.w_off));
        ch.wp2 = reinterpret_cast<const u32x4 *>(c.P(c2.w_off));
        ch.bias1 = c.P(c1.b_off);
        ch.bias2 = c.P(c2.b_off);
        ch.wscale1 = c1.wscale;
        ch.wscale2 = c2.wscale;
        ch.K1 = c1.K;
        ch.dil1 = c1.dil;
        ch.K2 = c2.K;
        ch.dil2 = c2.dil;
        macs += c1.macs_per_t + c2.macs_per_t;
        bytes += 4.0 * ((double)(c1.Cin + c1.Cout) + (double)(c2.Cin + c2.Cout));  // (layer-granular, as the separate launches)
    }
    vits_handle *h = c.h;
    a.rag = c.rag_at(T);
    a.peak = range_slots(h, true);
    macs *= c.work_frac();
    bytes *= c.work_frac();
    const bool ev = conv_event_begin(c);
    c.note(launch_conv_sx_mrf(a, c.B, c.st));
    fused_launch_end(c, ev, members, 2 * n, stg.rbs[n - 1].c1[0], T, 2.0 * macs * (double)T * c.B, bytes * T * c.B);
}

// Pinned output buffer of `bytes` bytes: the handle's pool when it is free (grown on demand), else a fresh
// allocation (the caller still holds an earlier output).  Released by pinned_put().
void *pinned_get(vits_handle *h, size_t bytes) {
    PinnedPool &p = h->pin;
    if (!p.busy) {
        if (bytes > p.cap) {
            if (p.base) hipHostFree(p.base);
            p.base = nullptr;
            p.cap = 0;
            size_t want = bytes + bytes / 4 + 4096;
            if (hipHostMalloc((void **)&p.base, want) != hipSuccess) return nullptr;
            p.cap = want;
        }
        p.busy = true;
        return p.base;
    }
    void *q = nullptr;
    return hipHostMalloc(&q, bytes) == hipSuccess ? q : nullptr;
}

void pinned_put(vits_handle *h, void *q) {
    if (!q) return;
    if (h && q == h->pin.base) h->pin.busy = false;
    else hipHostFree(q);
}

// The text-side kernels of the encoder and the stochastic duration predictor (kernels.hip.hpp): LayerNorm, the DDSConv layers,
// ConvFlow.pre, the spline and the ElementwiseAffine.  As with the token-to-frame kernels above, the pipeline and the kernel-level
// test hooks (vits_test_layernorm ...) launch through these, so each instantiation's choice and grid are stated once.
// LayerNorm over channels.  form: 16 or 32 time steps per workgroup of ln_tile_kernel (C <= 256), or one lane per column
// (layernorm_c_kernel, any C).  planes (tile forms with C % 8 == 0 only): the result once more as fp16 operand planes, `peak` =
// the range-guard slots of that conversion.
enum LnForm : int { LN_FORM_TILE16 = 0, LN_FORM_TILE32 = 1, LN_FORM_COLUMN = 2 };
void launch_layernorm(hipStream_t st, int form, int B, int C, int T, const float *in, float *out, const float *gamma,
                      const float *beta, const int *len, int flags, uint16_t *planes, unsigned *peak) {
    if (form == LN_FORM_TILE16 && planes)
        ln_tile_kernel<0, true, 16><<<dim3((T + 15) / 16, B), 256, 0, st>>>(in, out, gamma, beta, len, C, T, flags, nullptr, nullptr, 1, 1,
                                                                              planes, peak);
    else if (form == LN_FORM_TILE32 && planes)
        ln_tile_kernel<0, true><<<dim3((T + 31) / 32, B), 256, 0, st>>>(in, out, gamma, beta, len, C, T, flags, nullptr, nullptr, 1, 1,
                                                                          planes, peak);
    else if (form == LN_FORM_TILE16)
        ln_tile_kernel<0, false, 16><<<dim3((T + 15) / 16, B), 256, 0, st>>>(in, out, gamma, beta, len, C, T, flags, nullptr, nullptr, 1, 1);
    else if (form == LN_FORM_TILE32)
        ln_tile_kernel<0><<<dim3((T + 31) / 32, B), 256, 0, st>>>(in, out, gamma, beta, len, C, T, flags, nullptr, nullptr, 1, 1);
    else
        layernorm_c_kernel<<<dim3((T + 63) / 64, B), 64, 0, st>>>(in, out, gamma, beta, len, C, T, flags);
}

// out = GELU(LN(depthwise conv of in * mask)) (modules.py:121-123): the first third of an unfused DDSConv layer
void launch_dw_ln(hipStream_t st, int B, int C, int T, int K, int dil, const float *in, float *out, const float *dw_w,
                  const float *dw_b, const float *gamma, const float *beta, const int *len) {
    if (C <= 256 && K == 3)
        ln_tile_kernel<3><<<dim3((T + 31) / 32, B), 256, 0, st>>>(in, out, gamma, beta, len, C, T, LN_GELU, dw_w, dw_b, K, dil);
    else if (C <= 256)
        ln_tile_kernel<1><<<dim3((T + 31) / 32, B), 256, 0, st>>>(in, out, gamma, beta, len, C, T, LN_GELU, dw_w, dw_b, K, dil);
    else
        dds_dw_ln_gelu_kernel<<<dim3((T + 63) / 64, B), 64, 0, st>>>(in, out, dw_w, dw_b, gamma, beta, len, C, T, K, dil);
}

// one fused DDSConv layer, nblk = C / 32: 16 columns per workgroup (nblk 2, 4, 6, 8) ...
void launch_dds_layer16(hipStream_t st, int B, int nblk, const DdsLayer16Args &q) {
    const dim3 dg16((q.T + 15) / 16, B);
    switch (nblk) {
        case 2: dds_layer16_kernel<2><<<dg16, 256, 0, st>>>(q); break;
        case 4: dds_layer16_kernel<4><<<dg16, 256, 0, st>>>(q); break;
        case 6: dds_layer16_kernel<6><<<dg16, 256, 0, st>>>(q); break;
        default: dds_layer16_kernel<8><<<dg16, 256, 0, st>>>(q); break;
    }
}

// ... or 32 (nblk 1, 2, 3, 4, 6, 8)
void launch_dds_layer32(hipStream_t st, int B, int nblk, const DdsLayerArgs &a) {
    const dim3 dg((a.T + 31) / 32, B);
    switch (nblk) {  // (channel count at compile time: straight-line channel loops)
        case 1: dds_layer_kernel<1><<<dg, 256, 0, st>>>(a); break;
        case 2: dds_layer_kernel<2><<<dg, 256, 0, st>>>(a); break;
        case 3: dds_layer_kernel<3><<<dg, 256, 0, st>>>(a); break;
        case 4: dds_layer_kernel<4><<<dg, 256, 0, st>>>(a); break;
        case 6: dds_layer_kernel<6><<<dg, 256, 0, st>>>(a); break;
        default: dds_layer_kernel<8><<<dg, 256, 0, st>>>(a); break;
    }
}

void launch_cf_pre(hipStream_t st, int B, int C, int T, const float *z, int ch, const float *w, const float *bias, const float *cond,
                   float *h) {
    cf_pre_kernel<<<dim3((T + 255) / 256, C, B), 256, 0, st>>>(z, ch, w, bias, cond, h, C, T);
}

void launch_rqs_inverse(hipStream_t st, int B, int T, int nb, const float *pr, float *z, const int *len, int ch0, int ch1,
                        float sqrt_c) {
    if (nb <= 10) rqs_inverse_kernel<10><<<dim3((T + 63) / 64, B), 64, 0, st>>>(pr, z, len, ch0, ch1, nb, T, sqrt_c);
    else rqs_inverse_kernel<16><<<dim3((T + 63) / 64, B), 64, 0, st>>>(pr, z, len, ch0, ch1, nb, T, sqrt_c);
}

void launch_ea_logw(hipStream_t st, int B, int T, const float *z, int ch, float m0, float logs0, const int *len, float *logw) {
    ea_logw_kernel<<<dim3((T + 63) / 64, B), 64, 0, st>>>(z, ch, m0, logs0, len, logw, T);
}

// planes (optional): the result once more as fp16 operand planes of the split-operand engine (see split_planes)
void layernorm(Ctx &c, const float *in, float *out, int64_t g, int64_t b, const int *len, int C, int T, int flags,
               uint16_t *planes = nullptr) {
    // (16 time steps per workgroup: VITSMI_LN_TS=32 keeps the 32-step form, A/B timing)
    static const bool ts32 = [] { const char *e = std::getenv("VITSMI_LN_TS"); return e && std::atoi(e) == 32; }();
    const int form = C > 256 ? LN_FORM_COLUMN : (ts32 ? LN_FORM_TILE32 : LN_FORM_TILE16);
    const bool fused_planes = planes && C <= 256 && C % 8 == 0;
    launch_layernorm(c.st, form, c.B, C, T, in, out, c.P(g), c.P(b), len, flags, fused_planes ? planes : nullptr,
                     fused_planes ? range_slots(c.h, true) : nullptr);
    c.note(hipGetLastError());
    c.h->stats.total_launches++;
    if (planes && !fused_planes) split_planes(c, out, planes, C, T, nullptr);
}

// A stack of fused DDSConv layers over raw device pointers.  One launch per layer, ping-ponging between the three buffers
// hbuf, y, y2 ([B][C][T] each) so that the result of the last layer lands in hbuf: each layer must write a buffer other than
// the one it reads.  layer16: dds_layer16_kernel (C / 32 in {2, 4, 6, 8}), else dds_layer_kernel (1, 2, 3, 4, 6, 8).
// head, tail (layer16 only, optional): see ddsconv().  With a tail hbuf does NOT receive the stack's result.
struct DdsLayerPtrs {
    const float *dw_w, *dw_b, *ln1_g, *ln1_b, *ln2_g, *ln2_b;
    const float *pw_bias;  // [C]
    const float *pw16;     // layer16: the 1 x 1 weights in dds_layer16_kernel's A-operand layout
    const float *pw;       // layer32: ... packed for the conv engine (pack_conv), with that packing's geometry
    int CK, nchunks, MB;
    int dil;
};
struct DdsHead {
    const float *in, *z, *w, *b;  // conditioning tensor [B][C][T], z channel row of utterance 0 (rows 2 T apart), pre weights
};
struct DdsTail {
    const float *w16, *b;  // [ceil(rows / 16) * 16][C] in the pw16 layout, bias [rows] or nullptr
    float *out;            // [B][rows][T]
    int rows;
};
// 32-row blocks per m-tile of a conv-engine packing (DdsLayerPtrs::MB)
int dds_pw_blocks(const ConvDesc &pw) { return (pw.cfg == 2 ? 128 : ((pw.cfg == 1 || pw.cfg == 3) ? 64 : 32)) / 32; }
hipError_t launch_dds_stack(hipStream_t st, bool layer16, int B, int C, int T, int n_layers, const DdsLayerPtrs *layers, float *hbuf,
                            float *y, float *y2, const int *len, const DdsHead *head, const DdsTail *tail) {
    const int nblk = C / 32;
    float *bufs[3] = {hbuf, y, y2};
    int cur = 0;
    hipError_t err = hipSuccess;
    auto note = [&](hipError_t e) {
        if (err == hipSuccess) err = e;
    };
    for (int l = 0; l < n_layers; l++) {
        const DdsLayerPtrs &L = layers[l];
        const int left = n_layers - 1 - l;            // layers after this one
        int nxt = left == 0 ? 0 : (cur == 1 ? 2 : 1); // last layer writes hbuf ...
        if (nxt == cur) {                             // ... unless it would read it too (n_layers == 1): detour
            nxt = 1;
        }
        if (layer16) {
            DdsLayer16Args q{};
            q.in = bufs[cur];
            q.out = bufs[nxt];
            if (l == 0 && head) {
                q.in = head->in;
                q.head_z = head->z;
                q.head_w = head->w;
                q.head_b = head->b;
                q.head_zstride = (int64_t)2 * T;
            }
            q.len = len;
            q.dw_w = L.dw_w;
            q.dw_b = L.dw_b;
            q.ln1_g = L.ln1_g;
            q.ln1_b = L.ln1_b;
            q.ln2_g = L.ln2_g;
            q.ln2_b = L.ln2_b;
            q.pw16 = L.pw16;
            q.pw_bias = L.pw_bias;
            q.T = T;
            q.dil = L.dil;
            q.mask_out = left == 0;
            if (left == 0 && tail) {
                q.tail_w16 = tail->w16;
                q.tail_b = tail->b;
                q.tail_out = tail->out;
                q.tail_rows = tail->rows;
                q.tail_mask = 1;
            }
            launch_dds_layer16(st, B, nblk, q);
        } else {
            DdsLayerArgs a{};
            a.in = bufs[cur];
            a.out = bufs[nxt];
            a.len = len;
            a.dw_w = L.dw_w;
            a.dw_b = L.dw_b;
            a.ln1_g = L.ln1_g;
            a.ln1_b = L.ln1_b;
            a.ln2_g = L.ln2_g;
            a.ln2_b = L.ln2_b;
            a.pw = L.pw;
            a.pw_bias = L.pw_bias;
            a.C = C;
            a.T = T;
            a.dil = L.dil;
            a.mask_out = left == 0;
            a.CK = L.CK;
            a.nchunks = L.nchunks;
            a.MB = L.MB;
            launch_dds_layer32(st, B, nblk, a);
        }
        note(hipGetLastError());
        cur = nxt;
    }
    if (cur != 0 && !(layer16 && tail)) note(hipMemcpyAsync(hbuf, bufs[cur], (size_t)B * C * T * 4, hipMemcpyDeviceToDevice, st));
    return err;
}

// DDSConv (modules.py:117-129) in place on h [B,C,T]; y,y2 are scratch of the same size.
// tail (optional): the masked 1 x 1 conv `tail` (weights once more at tail16 in the 16-column kernel's layout) applied to the
// stack's result inside the last layer's launch, written to tail_out [B][tail->Cout][T]; hbuf does then NOT receive the stack's
// result.  Returns whether the tail was taken (false: the caller runs the conv itself).
// head (optional, ConvFlow stacks): the stack's input is head->w[c] * z + head->b[c] + head->in (ConvFlow.pre + conditioning),
// formed by the first layer while it loads; hbuf is then never read.  The caller asks dds16_head_ok() whether that form is
// taken; where it is not, it fills hbuf itself (launch_cf_pre) and passes no head.
// The form by width: C <= 256 with C / 32 in {2, 4, 6, 8} runs dds_layer16_kernel (VITSMI_DDS16=0: the 32-column kernel, A/B
// timing), 32 and 96 channels dds_layer_kernel, every other width (160 and 224 among them) the three launches per layer below.
bool dds16_head_ok(const DDSDesc &d, int C) {
    static const bool off = [] { const char *e = std::getenv("VITSMI_DDS16"); return e && e[0] == '0'; }();
    static const bool head_off = [] { const char *e = std::getenv("VITSMI_DDS_HEAD"); return e && e[0] == '0'; }();  // A/B timing only
    static const bool unfused = std::getenv("VITSMI_DDS_UNFUSED") != nullptr;
    const int nblk = C / 32;
    return !off && !head_off && !unfused && C <= 256 && C % 32 == 0 && d.K == 3 && d.n_layers > 1 && d.l[0].pw16 >= 0 &&
           (nblk == 2 || nblk == 4 || nblk == 6 || nblk == 8);
}
bool ddsconv(Ctx &c, const DDSDesc &d, float *hbuf, float *y, float *y2, const int *len, int C, int T,
             const ConvDesc *tail = nullptr, int64_t tail16 = -1, float *tail_out = nullptr, const DdsHead *head = nullptr) {
    static const bool unfused = std::getenv("VITSMI_DDS_UNFUSED") != nullptr;  // A/B timing only
    static const bool tail_off = [] { const char *e = std::getenv("VITSMI_DDS_TAIL"); return e && e[0] == '0'; }();  // A/B timing only
    static const bool dds16_off = [] { const char *e = std::getenv("VITSMI_DDS16"); return e && e[0] == '0'; }();
    const int nblk = C / 32;
    if (!unfused && C <= 256 && C % 32 == 0 && nblk != 5 && nblk != 7 && d.K == 3 && d.n_layers > 0) {
        bool layer16 = !dds16_off && (nblk == 2 || nblk == 4 || nblk == 6 || nblk == 8);
        DdsLayerPtrs layers[4];
        for (int l = 0; l < d.n_layers; l++) {
            const auto &L = d.l[l];
            layer16 = layer16 && L.pw16 >= 0;
            layers[l] = {c.P(L.dw_w), c.P(L.dw_b), c.P(L.ln1_g), c.P(L.ln1_b), c.P(L.ln2_g), c.P(L.ln2_b),
                         L.pw.b_off >= 0 ? c.P(L.pw.b_off) : c.P(c.m.zeros_off), L.pw16 >= 0 ? c.P(L.pw16) : nullptr,
                         c.P(L.pw.w_off), L.pw.CK, L.pw.nchunks, dds_pw_blocks(L.pw), L.dil};
            // the 1x1 conv's algorithmic work, as conv() would account it
            const double fl = 2.0 * L.pw.macs_per_t * (double)T * c.B;
            c.h->stats.conv_flops += fl;
            (c.h->cur_stage == 1 ? c.h->stats.dp_flops : c.h->stats.enc_flops) += fl;
        }
        DdsTail tl{};
        const bool tail_done = layer16 && tail && tail16 >= 0 && tail_out && !tail_off && tail->Cin == C && tail->K == 1 && tail->Cout <= C;
        if (tail_done) {
            tl = {c.P(tail16), tail->b_off >= 0 ? c.P(tail->b_off) : nullptr, tail_out, tail->Cout};
            const double tfl = 2.0 * tail->macs_per_t * (double)T * c.B;  // (accounted as conv() would)
            c.h->stats.conv_flops += tfl;
            (c.h->cur_stage == 1 ? c.h->stats.dp_flops : c.h->stats.enc_flops) += tfl;
        }
        // (head: dds16_head_ok - the caller checked that the 16-column path is taken)
        c.note(launch_dds_stack(c.st, layer16, c.B, C, T, d.n_layers, layers, hbuf, y, y2, len, layer16 ? head : nullptr,
                                tail_done ? &tl : nullptr));
        c.h->stats.total_launches += d.n_layers;
        return tail_done;
    }
    for (int l = 0; l < d.n_layers; l++) {
        const auto &L = d.l[l];
        launch_dw_ln(c.st, c.B, C, T, d.K, L.dil, hbuf, y, c.P(L.dw_w), c.P(L.dw_b), c.P(L.ln1_g), c.P(L.ln1_b), len);
        c.note(hipGetLastError());
        c.h->stats.total_launches++;
        conv(c, L.pw, y, (int64_t)C * T, T, y2, (int64_t)C * T, 0);
        int fl = LN_GELU | LN_ACCUM | (l == d.n_layers - 1 ? LN_MASK : 0);
        layernorm(c, y2, hbuf, L.ln2_g, L.ln2_b, len, C, T, fl);
    }
    return false;
}

void stage_mark(vits_handle *h, int idx) {
    if (h->timing) hipEventRecord(h->ev[idx], h->stream);
}

// The synthesis settings of a run: the call's one [3] vector (noise_scale, length_scale, noise_w) for every utterance, or
// (vits_run_*_rows) a host [B][3] row per utterance and optionally a host [B] of per-utterance noise seeds.  run_tokens
// copies the rows and seeds into the token slab; kernels read them there (d_rows / d_seeds), or take the call's scalars
// when d_rows is NULL.
struct RunRows {
    const float *scales = nullptr;  // host [3] (rows == false) or [B][3]
    bool rows = false;
    const uint64_t *seeds = nullptr;  // host [B] or NULL: the flat stream
    // vits_controls (validated on the host by host_controls): forced durations, or a per-token rate - never both
    const int64_t *durations = nullptr;  // host [B][T] or NULL
    const float *token_rate = nullptr;   // host [B][T] or NULL
    const float *d_rows = nullptr;
    const uint64_t *d_seeds = nullptr;
    const int64_t *d_durations = nullptr;
    const float *d_token_rate = nullptr;
    // vits_intonation (validated by vits_run_async_warped): host [B][T] semitones of a run that is warped, and its host lens
    // (vits_contour: semitones_end is set only where some token glides - the run then plans and launches the glide)
    const float *semitones = nullptr;
    const float *semitones_end = nullptr;
    const int64_t *semitone_lens = nullptr;
    // vits_fit (validated by host_fit; NULL when no row belongs to a group: the run is then the entry without a fit)
    const vits_fit *fit = nullptr;
    float at(int b, int col) const { return scales[(rows ? (int64_t)b * 3 : 0) + col]; }
    bool any(int B, int col) const {  // some utterance's value is not 0
        for (int b = 0; b < (rows ? B : 1); b++)
            if (at(b, col) != 0.f) return true;
        return false;
    }
};

// ---- token-domain part: encoder + duration predictor + durations.  Leaves y_len on the host.
int run_tokens(vits_handle *h, const int64_t *d_ids, const int64_t *d_lens, int B, int T, RunRows &rr,
               const int64_t *d_sid, const float *d_noise_dp, uint64_t seed) {
    const Model &m = h->model;
    const int H = m.H, C = m.C;
    TokenBufs w;
    if (int rc = slab_carve(h, h->tok, "token", [&](Carver &cv) { w = carve_tokens(cv, m, B, T); })) return rc;
    Ctx c{h, m, h->stream, h->arena_dev, B};
    hipStream_t st = h->stream;

    h->d_len = w.len;
    h->d_ylen64 = w.ylen64;
    h->d_cum = w.cum;
    float *x = w.x, *att = w.att, *xe = w.xe, *qkv = w.qkv, *ffh = w.ffh, *stats = w.stats;
    h->d_emb = xe;
    h->d_x = x;
    h->d_logw = w.logw;
    h->d_wceil = w.wceil;
    h->d_ylen = reinterpret_cast<int *>(h->d_wceil + (size_t)B * T);

    if (rr.rows) {
        HIPCHECK(h, hipMemcpyAsync(w.rows, rr.scales, sizeof(float) * 3 * B, hipMemcpyHostToDevice, st));
        rr.d_rows = w.rows;
    }
    if (rr.seeds) {
        HIPCHECK(h, hipMemcpyAsync(w.seeds, rr.seeds, sizeof(uint64_t) * B, hipMemcpyHostToDevice, st));
        rr.d_seeds = w.seeds;
    }
    if (rr.durations) {
        HIPCHECK(h, hipMemcpyAsync(w.ctl, rr.durations, sizeof(int64_t) * B * T, hipMemcpyHostToDevice, st));
        rr.d_durations = w.ctl;
    } else if (rr.token_rate) {
        float *d = reinterpret_cast<float *>(w.ctl);
        HIPCHECK(h, hipMemcpyAsync(d, rr.token_rate, sizeof(float) * B * T, hipMemcpyHostToDevice, st));
        rr.d_token_rate = d;
    }
    const bool forced = rr.d_durations != nullptr;
    h->last_forced = forced;
    h->h_dur_B = h->h_dur_T = 0;
    h->h_fit.clear();
    h->d_fit_w = nullptr;
    const int G = rr.fit ? rr.fit->n_groups : 0;  // (host_fit: G <= B, every id and target checked)
    std::vector<int64_t> in;  // (pageable, and read by the copy below: it lives until this function's one synchronisation)
    if (G > 0) {
        // [target int64 B | group int32 B | mode int32 B] gathered on the host and sent as one copy
        in.assign((size_t)B * 2, 0);
        int32_t *gm = reinterpret_cast<int32_t *>(in.data() + B);
        for (int g = 0; g < G; g++) in[g] = rr.fit->target_frames[g], gm[B + g] = rr.fit->mode[g];
        for (int b = 0; b < B; b++) gm[b] = rr.fit->group[b];
        HIPCHECK(h, hipMemcpyAsync(w.fit_in, in.data(), sizeof(int64_t) * 2 * B, hipMemcpyHostToDevice, st));
    }
    lens_to_i32<<<(B + 63) / 64, 64, 0, st>>>(d_lens, h->d_len, B, T);
    const int *len = h->d_len;
    h->cur_stage = 0;
    stage_mark(h, 0);
    embed_kernel<<<dim3((T + 63) / 64, (H + 15) / 16, B), 64, 0, st>>>(d_ids, len, c.P(m.emb), xe, H, T, m.n_vocab,
                                                        (float)std::sqrt((double)H));
    h->stats.total_launches += 2;
    const int64_t sHT = (int64_t)H * T;
    const float *xin = xe;  // layer input: the embedding for layer 0, x afterwards
    ConvOpt masked;         // the convs whose flags mask by the token counts
    masked.len = len;
    SxOpt masked_sx;
    masked_sx.len = len;
    // split-operand engine (Model::enc_sx): every conv reads fp16 operand planes and writes planar fp32 (what attention,
    // LayerNorm and the duration predictor read) or planes for the next conv
    uint16_t *x_pl = w.x_pl, *att_pl = w.att_pl, *ff_pl = w.ff_pl, *qkv_pl = w.qkv_pl;
    if (m.enc_sx) split_planes(c, xe, x_pl, H, T, len);
    for (auto &L : m.enc) {
        if (m.enc_sx) {
            const bool a16 = attention16_ok(m.dk, m.window);
            conv_sx_planar(c, L.qkv_sx, x_pl, T, a16 ? nullptr : qkv, a16 ? qkv_pl : nullptr, 0);  // (a16 reads the planes only)
            // (the attention kernel writes its output as conv_o's operand planes too when head widths are whole cells)
            uint16_t *apl = m.dk % 8 == 0 ? att_pl : nullptr;
            if (a16)
                c.note(launch_attention16(st, B, T, m.n_heads, m.dk, m.window, qkv_pl, nullptr, apl, c.P(L.rel_k), c.P(L.rel_v), len,
                                          H, range_slots(h, true)));
            else
                launch_attention(st, B, T, m.n_heads, m.dk, m.window, qkv, att, c.P(L.rel_k), c.P(L.rel_v), len, H, apl,
                                 apl ? range_slots(h, true) : nullptr);
            c.note(hipGetLastError());
            h->stats.total_launches++;
            h->stats.enc_flops += 2.0 * B * m.n_heads * (2.0 * m.dk * T * (double)T);
            if (!apl) split_planes(c, att, att_pl, H, T, nullptr);
            SxOpt ores;
            ores.res = xin;
            conv_sx_planar(c, L.o_sx, att_pl, T, x, nullptr, EPI_RES, ores);
            xin = x;
            layernorm(c, x, x, L.ln1_g, L.ln1_b, len, H, T, LN_MASK, x_pl);
            conv_sx_planar(c, L.ffn1_sx, x_pl, T, nullptr, ff_pl, EPI_RELU | EPI_MASK, masked_sx);
            conv_sx_planar(c, L.ffn2_sx, ff_pl, T, x, nullptr, EPI_MASK | EPI_ACC, masked_sx);
            layernorm(c, x, x, L.ln2_g, L.ln2_b, len, H, T, LN_MASK, x_pl);
            continue;
        }
        // q|k|v = 1x1 convs (attentions.py:216-218), fused into one [3H,H] GEMM
        conv(c, L.qkv, xin, sHT, T, qkv, 3 * sHT, 0);
        launch_attention(st, B, T, m.n_heads, m.dk, m.window, qkv, att, c.P(L.rel_k), c.P(L.rel_v), len, H);
        c.note(hipGetLastError());
        h->stats.total_launches++;
        h->stats.enc_flops += 2.0 * B * m.n_heads * (2.0 * m.dk * T * (double)T);
        // x = LN(x + conv_o(att))  (attentions.py:66-68)
        ConvOpt ores;
        ores.res = xin;
        ores.res_bstride = sHT;
        conv(c, L.o, att, sHT, T, x, sHT, EPI_RES, ores);
        xin = x;
        // Padded positions never reach valid ones (keys are masked, every other op is per-position or reads
        // x*mask), so masking the LayerNorm outputs changes no observable value and lets the FFN convs read
        // their input without a ragged mask (16-byte LDS-DMA path).
        layernorm(c, x, x, L.ln1_g, L.ln1_b, len, H, T, LN_MASK);
        // FFN (attentions.py:386-407): conv(x*mask) -> relu -> conv(h*mask) -> *mask ; x = LN(x + y)
        conv(c, L.ffn1, x, sHT, T, ffh, (int64_t)m.FF * T, EPI_RELU | EPI_MASK, masked);
        ConvOpt ffn_res = masked;
        ffn_res.res = x;
        ffn_res.res_bstride = sHT;
        conv(c, L.ffn2, ffh, (int64_t)m.FF * T, T, x, sHT, EPI_MASK | EPI_RES, ffn_res);
        layernorm(c, x, x, L.ln2_g, L.ln2_b, len, H, T, LN_MASK);
    }
    // x = x * mask ; stats = proj(x) * mask (models.py:205-208)
    mask_kernel<<<dim3((T + 255) / 256, H, B), 256, 0, st>>>(x, len, H, T);
    h->stats.total_launches++;
    if (m.enc_sx) conv_sx_planar(c, m.enc_proj_sx, x_pl, T, stats, nullptr, EPI_MASK, masked_sx);
    else conv(c, m.enc_proj, x, sHT, T, stats, (int64_t)2 * C * T, EPI_MASK, masked);
    h->d_mp = stats;                       // [B, 2C, T] : m_p = rows [0,C), logs_p = rows [C,2C)
    h->d_logs = stats + (int64_t)C * T;    // batch stride 2*C*T for both

    // ---- speaker conditioning vectors
    float *dp_cond = nullptr;
    if (m.gin && !d_sid) return fail(h, VITS_E_ARG, "Missing speaker id");
    if (m.gin && !forced) {
        dp_cond = w.dp_cond;
        cond_matvec_kernel<<<dim3((m.dp_cond_rows + 63) / 64, B), 64, 0, st>>>(
            c.P(m.emb_g), d_sid, m.n_speakers, c.P(m.dp_cond_w), c.P(m.dp_cond_b), dp_cond, m.dp_cond_rows, m.gin);
        h->stats.total_launches++;
    }

    // ---- duration predictor
    h->cur_stage = 1;
    stage_mark(h, 1);
    const float noise_w = rr.at(0, 2);
    if (forced) {
        // forced durations: the duration predictor - stochastic or plain, its convs, spline flows and noise - is not
        // launched at all, and there is no logw (tap "logw" says so)
        h->d_logw = nullptr;
    } else if (m.use_sdp) {
        const int Cd = m.dp_pre.Cout;
        const int64_t sC = (int64_t)Cd * T;
        float *hb = w.hb, *y = w.y, *y2 = w.y2, *cond = w.cond, *h2 = w.h2, *pr = w.pr, *z = w.z;
        // h = pre(x) [+ cond(g)] ; DDSConv ; cond = proj(h)*mask (models.py:65-70)
        ConvOpt cond_bias;
        cond_bias.bias_b = dp_cond;
        cond_bias.bias_b_stride = m.dp_cond_rows;
        conv(c, m.dp_pre, x, sHT, T, hb, sC, 0, cond_bias);
        if (!ddsconv(c, m.dp_convs, hb, y, y2, len, Cd, T, &m.dp_proj, m.dp_proj16, cond))
            conv(c, m.dp_proj, hb, sC, T, cond, sC, EPI_MASK, masked);
        // z = randn * noise_scale_w (models.py:111), per utterance: +0.0 where noise_w is 0
        int64_t nz = (int64_t)B * 2 * T;
        if (!rr.any(B, 2)) {
            c.note(hipMemsetAsync(z, 0, nz * 4, st));
        } else if (d_noise_dp) {
            scale_kernel<<<(unsigned)((nz + 255) / 256), 256, 0, st>>>(d_noise_dp, z, noise_w, rr.d_rows, 2, 2 * T, nz);
        } else if (rr.d_seeds) {
            launch_fill_normal_rows(st, B, 2, T, z, rr.d_seeds, 1u, rr.d_rows, 2);
        } else {
            launch_fill_normal(st, z, nz, seed, 1);
            scale_kernel<<<(unsigned)((nz + 255) / 256), 256, 0, st>>>(z, z, noise_w, rr.d_rows, 2, 2 * T, nz);
        }
        h->stats.total_launches += 2;
        int swapped = 0;  // logical channel 0 lives in physical channel `swapped`
        for (int f = 0; f < 3; f++) {
            swapped ^= 1;  // Flip (modules.py:384-391)
            const auto &cf = m.cf[f];
            int ch0 = swapped, ch1 = swapped ^ 1;
            DdsHead hd{cond, z + (int64_t)ch0 * T, c.P(cf.pre_w), c.P(cf.pre_b)};
            const bool use_head = dds16_head_ok(cf.convs, Cd);
            if (!use_head) {
                launch_cf_pre(st, B, Cd, T, z, ch0, c.P(cf.pre_w), c.P(cf.pre_b), cond, h2);
                h->stats.total_launches++;
            }
            if (!ddsconv(c, cf.convs, h2, y, y2, len, Cd, T, &cf.proj, cf.proj16, pr, use_head ? &hd : nullptr))
                conv(c, cf.proj, h2, sC, T, pr, (int64_t)cf.proj.Cout * T, EPI_MASK, masked);
            float sqc = std::sqrt((float)Cd);
            launch_rqs_inverse(st, B, T, cf.nb, pr, z, len, ch0, ch1, sqc);
            c.note(hipGetLastError());
            h->stats.total_launches++;
        }
        swapped ^= 1;
        launch_ea_logw(st, B, T, z, swapped, m.ea_m0, m.ea_logs0, len, h->d_logw);
        h->stats.total_launches++;
    } else {
        const int Fd = m.dpp_F;
        float *xi = x;
        if (dp_cond) {  // x = x + cond(g) (models.py:153-155)
            xi = w.xi;
            add_bias_b_kernel<<<dim3((T + 255) / 256, H, B), 256, 0, st>>>(x, xi, dp_cond, m.dp_cond_rows, H, T);
            h->stats.total_launches++;
        }
        float *h1 = w.h1, *h2 = w.h2;
        const int64_t sF = (int64_t)Fd * T;
        conv(c, m.dpp_conv1, xi, sHT, T, h1, sF, PRO_MASK | EPI_RELU, masked);
        layernorm(c, h1, h1, m.dpp_n1_g, m.dpp_n1_b, len, Fd, T, 0);
        conv(c, m.dpp_conv2, h1, sF, T, h2, sF, PRO_MASK | EPI_RELU, masked);
        layernorm(c, h2, h2, m.dpp_n2_g, m.dpp_n2_b, len, Fd, T, 0);
        conv(c, m.dpp_proj, h2, sF, T, h->d_logw, T, PRO_MASK | EPI_MASK, masked);
    }
    // ---- durations (models.py:702-704)
    if (forced)
        launch_forced_durations(st, B, T, rr.d_durations, len, h->d_wceil, h->d_cum, h->d_ylen);
    else
        launch_durations(st, B, T, h->d_logw, len, rr.at(0, 1), rr.d_rows, rr.d_token_rate, h->d_wceil, h->d_cum, h->d_ylen);
    h->stats.total_launches++;
    c.note(hipGetLastError());
    const size_t nBT = (size_t)B * T;
    if (G > 0) {
        // fitted durations: the weights duration_kernel ceiled, then one workgroup per group that overwrites the fitted rows
        const int *gm = reinterpret_cast<const int *>(w.fit_in + B);
        launch_fit_weights(st, B, T, h->d_logw, len, rr.at(0, 1), rr.d_rows, rr.d_token_rate, w.fit_w);
        launch_fit_durations(st, B, T, G, w.fit_w, len, gm, w.fit_in, gm + B, h->d_wceil, h->d_cum, h->d_ylen,
                             reinterpret_cast<FitResult *>(h->d_wceil + fit_block_offset(nBT, B)));
        h->stats.total_launches += 2;
        c.note(hipGetLastError());
        h->d_fit_w = w.fit_w;
    }
    if (c.err != hipSuccess) return fail(h, VITS_E_DEVICE, "kernel launch failed: %s", hipGetErrorString(c.err));
    // the one data-dependent readback: the frame counts (output length) and, in the same copy, the durations themselves
    const size_t nrb = G > 0 ? fit_block_floats(nBT, B, G) : nBT + B;
    h->h_ylen.resize(B);
    h->h_dur.resize(nBT);
    if (h->h_rb_pin_n < nrb) {
        if (h->h_rb_pin) hipHostFree(h->h_rb_pin);
        h->h_rb_pin = nullptr;
        h->h_rb_pin_n = 0;
        const size_t cap = nrb < 16384 ? 16384 : nrb + nrb / 4;
        if (hipHostMalloc((void **)&h->h_rb_pin, sizeof(float) * cap) == hipSuccess) h->h_rb_pin_n = cap;
    }
    if (h->h_rb_pin_n >= nrb) {
        HIPCHECK(h, hipMemcpyAsync(h->h_rb_pin, h->d_wceil, sizeof(float) * nrb, hipMemcpyDeviceToHost, st));
        HIPCHECK(h, hipStreamSynchronize(st));
        std::memcpy(h->h_dur.data(), h->h_rb_pin, sizeof(float) * nBT);
        std::memcpy(h->h_ylen.data(), h->h_rb_pin + nBT, sizeof(int) * B);
        if (G > 0) {
            h->h_fit.resize(G);
            std::memcpy(h->h_fit.data(), h->h_rb_pin + fit_block_offset(nBT, B), sizeof(FitResult) * G);
        }
    } else {
        if (G > 0) {
            h->h_fit.resize(G);
            HIPCHECK(h, hipMemcpyAsync(h->h_fit.data(), h->d_wceil + fit_block_offset(nBT, B), sizeof(FitResult) * G, hipMemcpyDeviceToHost, st));
        }
        HIPCHECK(h, hipMemcpyAsync(h->h_dur.data(), h->d_wceil, sizeof(float) * nBT, hipMemcpyDeviceToHost, st));
        HIPCHECK(h, hipMemcpyAsync(h->h_ylen.data(), h->d_ylen, sizeof(int) * B, hipMemcpyDeviceToHost, st));
        HIPCHECK(h, hipStreamSynchronize(st));
    }
    h->h_dur_B = B;
    h->h_dur_T = T;
    if (h->range_pending) {  // an earlier asynchronous run whose range verdict nobody has looked at
        const vits_stats keep = h->stats;
        const int rr = range_check(h);
        h->stats = keep;
        if (rr) return fail(h, VITS_E_RANGE, "the previous run on this handle left the range of the fp16 operand planes");
    }
    int F = 1;
    for (int b = 0; b < B; b++) F = h->h_ylen[b] > F ? h->h_ylen[b] : F;
    h->F = F;
    return 0;
}

// Ragged rendering of a padded batch (vits_handle::tails_reference == false): from here on every generator launch ends
// utterance b's tensors gen_rf_frames behind ylen[b] (Ctx::rag_at), and the tail kernel writes zeros behind ylen[b] * hop.
// Needs the host copy of the frame counts (Ctx::h_len) for the FLOP / byte accounting; B = 1 has no padding.
// the margin of the following launches (frames behind an utterance's end that its tensors still cover), and with it the
// share of B * F frames they work on
void rag_margin(Ctx &c, int add) {
    if (!c.rag.len) return;
    const int B = c.B, F = c.rag_F;
    double cols = 0;
    for (int b = 0; b < B; b++) {
        const int n = c.h_len[b];
        cols += n > 0 ? (n + add < F ? n + add : F) : 0;
    }
    c.rag.add = add;
    c.rag_frac = cols / ((double)B * F);
}
void rag_begin(vits_handle *h, Ctx &c, const int *ylen, int B, int F) {
    c.rag = SxRagged{nullptr, 0, 0};
    c.rag_F = F;
    c.rag_frac = 1.0;
    if (!ylen || !c.h_len || B < 2 || B != c.B || h->tails_reference) return;
    c.rag = SxRagged{ylen, 0, 1};
    rag_margin(c, h->model.gen_rf_frames);  // (conv_pre: the whole receptive field; the stages set their own, smaller ones)
}
// the frame counts the tail kernel zeroes behind (nullptr: the reference's padded rendering is kept as it is)
const int *tail_len(const vits_handle *h, const int *ylen) { return h->tails_reference ? nullptr : ylen; }

// ---- the generator (models.py:348-368): three walkers over one dataflow, picked by run_generator() below.  Common to them:

// MRF accumulation (models.py:356-363) by the last step of ResBlock j of nk: xs = rb0(x); xs += rb1(x); ...; x = xs / nk
int mrf_flags(int j, int nk) { return (j == 0 ? 0 : EPI_ACC) | (j == nk - 1 && nk > 1 ? EPI_DIV : 0); }

// what one step of a ResBlock writes on the split-operand engine: epilogue flags, fp32 raw and plane destination
struct StepOut {
    int flags;
    float *raw;
    uint16_t *pl;
};

// conv_post's launch check and accounting
void conv_post_account(vits_handle *h, Ctx &c, int B, int T) {
    const Model &m = h->model;
    c.note(hipGetLastError());
    h->stats.total_launches++;
    const double fl = 2.0 * m.post_cin * m.post_k * (double)T * B * c.work_frac(), by = 4.0 * B * ((double)m.post_cin * T + T) * c.work_frac();
    h->stats.dec_flops += fl;
    h->stats.dec_bytes += by;
}

// leaky_relu(0.01), conv_post, tanh (models.py:364-366) from the fp32 raw stage output of the two split-operand walkers
void conv_post_sx(vits_handle *h, Ctx &c, const float *x, const int *ylen, int B, int T, int F, float *out) {
    const Model &m = h->model;
    hipStream_t st = h->stream;
    h->S = T;
    h->d_out = out;
    launch_post_conv_blocked(st, B, m.post_cin, m.post_k, T, x, c.P(m.post_w), h->d_out, 0.01f, tail_len(h, ylen), T / F);
    conv_post_account(h, c, B, T);
}

// The PLANE-STREAM generator of the two fp16 arithmetics (Model::gen_planes): f16 (VITSMI_GEN_PRECISION=f16, BASELINE config
// 4's reduced-precision vocoder: one fp16 plane per operand, one product) and, for A/B runs, f16x3 (VITSMI_F16X3_STREAM=planes:
// two planes, three MFMA products per fp32 product).  Every tensor between two convs exists ONCE, as the operand planes of the
// consumer's leaky_relu ([planes][C/8][T][8]: 4 / 2 bytes per element): a conv reads them as its B operand straight from LDS
// (by LDS-DMA), and a residual add recovers x from them by undoing the leaky_relu (x = p >= 0 ? p : p / 0.1; exact up to the
// planes' own resolution - 22 bits in f16x3).  No fp32 copy of the residual stream is written or read; only the
// multi-receptive-field sum xs (models.py:356-363; three read-modify-writes per stage) is fp32.  Everything in front of z is
// unchanged.  Same dataflow as run_generator_sx.
void run_generator_planes(vits_handle *h, Ctx &c, const float *z, int64_t z_bstride, int z_cstride, const int *ylen, int B,
                          int F, const float *dec_cond, const GenBufs &gb) {
    const Model &m = h->model;
    hipStream_t st = h->stream;
    // (plane tensors keep the three-slot batch stride of the other modes)
    uint16_t *const *stage_in = gb.stage_in, *y_pl = gb.y_pl, *const *raa = gb.raa, *tmp_pl = gb.tmp_pl;
    float *xs_raw = gb.xs_raw;
    rag_begin(h, c, ylen, B, F);
    const float S = 0.1f;  // Generator.LRELU_SLOPE / ResBlock LRELU_SLOPE
    const int nst = (int)m.ups.size();
    SxOpt act;  // every plane tensor is stored as leaky_relu(value, 0.1): what its consumer multiplies
    act.oslope2 = S;
    // z * y_mask (models.py:349) as conv_pre's operand plane (no activation in front of conv_pre)
    sx_split_planes_kernel<<<dim3((F + 255) / 256, m.C / 8, B), 256, 0, st>>>(z, z_bstride, z_cstride, ylen, tmp_pl, m.C, F,
                                                                              m.gen_h1 ? 2 : 1, range_slots(h, true));
    c.note(hipGetLastError());
    h->stats.total_launches++;
    // xa = leaky_relu(conv_pre(z) [+ cond(g)], 0.1) (models.py:349-354)
    SxOpt pre = act;
    pre.bias_b = dec_cond;
    pre.bias_b_stride = m.C0;
    conv_sx(c, m.conv_pre, tmp_pl, F, nullptr, stage_in[0], 0, pre);
    const uint16_t *xa = stage_in[0];
    int T = F;
    for (int si = 0; si < nst; si++) {
        const auto &stg = m.ups[si];
        rag_margin(c, m.gen_rf_stage[si]);  // (what is left of the receptive field from this stage's input on)
        // y = up(xa), stored as leaky_relu(y, 0.1): the resblocks' first operand and, un-activated, their residual
        conv_sx(c, stg.up, xa, T, nullptr, y_pl, 0, act);
        T *= stg.u;
        uint16_t *xs_pl = stage_in[(si + 1) & 1];
        const int nk = (int)stg.rbs.size();
        const bool last_stage = si == nst - 1;
        for (int j = 0; j < nk; j++) {
            const auto &rbk = stg.rbs[j];
            // Step q of this block writes its stream as planes; the last step the running sum xs instead (fp32).  The stage
            // output x = xs / nk feeds the next upsampler as a plane (leaky_relu 0.1) - with one block per stage there is
            // no sum to keep and no fp32 destination at all; the last stage's feeds conv_post as fp32 (its kernel applies
            // leaky_relu 0.01).
            auto step_out = [&](int q) {
                StepOut w{EPI_RES, nullptr, raa[q & 1]};
                if (q == rbk.n - 1) {
                    w.flags |= mrf_flags(j, nk);
                    w.raw = xs_raw;
                    w.pl = nullptr;
                    if (j == nk - 1 && !last_stage) {
                        w.pl = xs_pl;
                        if (nk > 1) w.flags |= SX_NO_RAW_STORE;
                        else w.raw = nullptr;
                    }
                }
                return w;
            };
            // flags of a fused launch: the multi-receptive-field arithmetic + which of the two destinations it writes
            auto p16_flags = [](const StepOut &w) {
                return (w.flags & (EPI_ACC | EPI_DIV)) | (w.raw && !(w.flags & SX_NO_RAW_STORE) ? P16_HAS_RAW : 0) | (w.pl ? P16_HAS_PL : 0);
            };
            const uint16_t *cur = y_pl;
            for (int q = 0; q < rbk.n; q++) {
                StepOut w = step_out(q);
                SxOpt res = act;  // a step's closing conv: + x, recovered from the planes of leaky_relu(x)
                res.div = (float)nk;
                res.res_pl = cur;
                res.res_slope = S;
                if (rbk.type1) {  // modules.py:301-314: x = c2(lrelu(c1(lrelu(x)))) + x
                    if (sx_pair16_ok(h, rbk.c1[q], rbk.c2[q]))
                        conv_sx_pair16(c, rbk.c1[q], rbk.c2[q], cur, T, w.raw, w.pl, p16_flags(w), (float)nk, S, false);
                    else {
                        conv_sx(c, rbk.c1[q], cur, T, nullptr, tmp_pl, 0, act);
                        conv_sx(c, rbk.c2[q], tmp_pl, T, w.raw, w.pl, w.flags, res);
                    }
                } else if (q + 1 < rbk.n && sx_pair16_ok(h, rbk.c1[q], rbk.c1[q + 1])) {
                    // modules.py:355-364, two steps in one launch: x1 = c(lrelu(x)) + x ; x = c'(lrelu(x1)) + x1
                    w = step_out(++q);
                    conv_sx_pair16(c, rbk.c1[q - 1], rbk.c1[q], cur, T, w.raw, w.pl, p16_flags(w), (float)nk, S, true);
                } else  // modules.py:355-364: x = c(lrelu(x)) + x
                    conv_sx(c, rbk.c1[q], cur, T, w.raw, w.pl, w.flags, res);
                cur = w.pl;
            }
        }
        xa = xs_pl;
    }
    conv_post_sx(h, c, xs_raw, ylen, B, T, F, gb.out);
}

// f16x3, plane-format stages: residual stream as operand planes only (run_generator_sx); VITSMI_F16X3_RES=raw for the fp32 one
bool res_planes_on() {  // (read per run: tests switch it inside one process)
    // default ON (r05e, same box, two runs each: 138.9 / 137.4 M samples/s against 136.3 / 136.3 with the fp32 residual stream;
    // 128-channel k = 3 residual conv 652 -> 588-600 us, stride-8 upsampler 983 -> 830 us, k = 11 residual convs +2-3 %)
    const char *e = std::getenv("VITSMI_F16X3_RES");
    return e ? std::string(e) != "raw" : true;
}

// The RAW-STREAM generator on the split-operand engine (f16x3, the default, and bf16x6).  Same dataflow as run_generator_f32
// below; tensors that feed a conv are stored as 16-bit planes (already leaky-ReLU'd by their producer), the residual stream as
// fp32 raw cells.
void run_generator_sx(vits_handle *h, Ctx &c, const float *z, int64_t z_bstride, int z_cstride, const int *ylen, int B,
                      int F, const float *dec_cond, const GenBufs &gb) {
    const Model &m = h->model;
    hipStream_t st = h->stream;
    uint16_t *const *stage_in = gb.stage_in, *y_pl = gb.y_pl, *const *raa = gb.raa, *tmp_pl = gb.tmp_pl;
    float *y_raw = gb.y_raw, *const *ra = gb.ra, *xs_raw = gb.xs_raw;
    // the plane regions double as fp32 raw buffers where a stage uses the raw format (plane_floats(R) >= R floats)
    float *tmp_raw = reinterpret_cast<float *>(tmp_pl), *xin_raw = reinterpret_cast<float *>(stage_in[0]);
    rag_begin(h, c, ylen, B, F);
    const float S = 0.1f;  // Generator.LRELU_SLOPE / ResBlock LRELU_SLOPE
    const int nst = (int)m.ups.size();
    // Tensor formats (model.hpp sx_raw_format): > 64 channels: 16-bit planes that already carry the consumer's
    // leaky_relu (+ fp32 raw where the tensor is also a residual); <= 64 channels: fp32 raw only, the consuming
    // conv applies the leaky_relu and the split while loading (its `islope`).
    SxOpt lrelu;  // a conv between tensors of either format: both slopes (each is read only where its tensor exists)
    lrelu.oslope2 = S;
    lrelu.islope = S;
    // ---- z * y_mask (models.py:349) in conv_pre's input format
    const void *zin;
    if (sx_raw_format(m.C)) {
        sx_block_kernel<<<dim3((F + 255) / 256, m.C / 8, B), 256, 0, st>>>(z, z_bstride, z_cstride, ylen, tmp_raw, m.C, F,
                                                                           range_slots(h, m.gen_f16));
        zin = tmp_raw;
    } else {
        sx_split_planes_kernel<<<dim3((F + 255) / 256, m.C / 8, B), 256, 0, st>>>(z, z_bstride, z_cstride, ylen, tmp_pl, m.C, F,
                                                                                  m.gen_f16 ? 1 : 0, range_slots(h, m.gen_f16));
        zin = tmp_pl;
    }
    c.note(hipGetLastError());
    h->stats.total_launches++;
    // ---- xa = conv_pre(z) [+ cond(g)]; leaky_relu(0.1) follows (models.py:349-354)
    SxOpt pre;
    pre.bias_b = dec_cond;
    pre.bias_b_stride = m.C0;
    const void *xa;
    if (sx_raw_format(m.C0)) {
        conv_sx(c, m.conv_pre, zin, F, xin_raw, nullptr, 0, pre);
        xa = xin_raw;
    } else {
        pre.oslope2 = S;
        conv_sx(c, m.conv_pre, zin, F, nullptr, stage_in[0], 0, pre);
        xa = stage_in[0];
    }
    int T = F;
    for (int si = 0; si < nst; si++) {
        const auto &stg = m.ups[si];
        rag_margin(c, m.gen_rf_stage[si]);  // (what is left of the receptive field from this stage's input on)
        const bool fr = sx_raw_format(stg.C);  // format of this stage's tensors
        SxOpt act;  // ... and with it who applies the leaky_relu between two of its convs: the consumer (raw) or the producer
        if (fr) act.islope = S;
        else act.oslope2 = S;
        // Plane-format stages (> 64 channels) in f16x3: the residual stream as operand planes ONLY (SX_RES_PL: a residual is
        // recovered from the planes of leaky_relu(x), 22 bits, as in run_generator_planes) - no fp32 copy of y and of the
        // blocks' intermediate x is written or read: 12 instead of 16 bytes per element on the residual convs, which at 128
        // channels and k = 3 are HBM-bound (launch table r05c: 0.65 ms = 4.9 TB/s of real traffic).  Needs every conv of the
        // stage on the 16x16x32 loop (the SX_RES_PL instantiations); VITSMI_F16X3_RES=raw keeps the fp32 residual stream (A/B).
        bool rpl = !fr && h->gen_nprod == 2 && res_planes_on() && stg.up.s16;
        for (const auto &rbk : stg.rbs)
            for (int q = 0; q < rbk.n && rpl; q++) rpl = rbk.c1[q].s16 && rbk.c1[q].f16 && (!rbk.type1 || (rbk.c2[q].s16 && rbk.c2[q].f16));
        // y = up(leaky_relu(xa)): pixel-shuffled dense conv; raw (residual / raw-format input) [+ planes]
        conv_sx(c, stg.up, xa, T, rpl ? nullptr : y_raw, fr ? nullptr : y_pl, 0, lrelu);
        T *= stg.u;
        uint16_t *xs_pl = stage_in[(si + 1) & 1];
        const int nk = (int)stg.rbs.size();
        const bool last_stage = si == nst - 1;
        if (fr && sx_mrf_ok(h, stg)) {
            // every ResBlock2 of the stage in one launch: x read once, the sum formed in registers, one store
            conv_sx_mrf(c, stg, y_raw, T, xs_raw, S);
            xa = xs_raw;
            continue;
        }
        for (int j = 0; j < nk; j++) {
            const auto &rbk = stg.rbs[j];
            // Step q of this block writes its stream raw and (plane format) as planes - as planes only where the residual is
            // taken from them (rpl); the last step the running sum xs instead.  The stage output x = xs / nk feeds the next
            // upsampler (leaky_relu 0.1) or conv_post (0.01): planes carry the activation, raw tensors get it from their
            // consumer.
            auto step_out = [&](int q) {
                StepOut w{EPI_RES, rpl ? nullptr : ra[q & 1], fr ? nullptr : raa[q & 1]};
                if (q == rbk.n - 1) {
                    w.flags |= mrf_flags(j, nk);
                    w.raw = xs_raw;
                    w.pl = nullptr;
                    if (j == nk - 1 && !last_stage && !fr) {
                        w.pl = xs_pl;
                        w.flags |= SX_NO_RAW_STORE;
                    }
                }
                return w;
            };
            const float *cur = y_raw;          // residual operand
            const uint16_t *cura = y_pl;       // plane format: leaky_relu(cur) as planes
            for (int q = 0; q < rbk.n; q++) {
                StepOut w = step_out(q);
                if (rbk.type1 && fr && sx_pair_ok(h, rbk.c1[q], rbk.c2[q])) {
                    // modules.py:301-314 in one launch: the intermediate stays in LDS, x is read once
                    conv_sx_pair(c, rbk.c1[q], rbk.c2[q], cur, T, w.raw, w.flags, (float)nk, S);
                } else if (!rbk.type1 && fr && q + 1 < rbk.n && sx_pair_ok(h, rbk.c1[q], rbk.c1[q + 1])) {
                    // modules.py:355-364, two steps in one launch: x1 = c(lrelu(x)) + x ; x = c'(lrelu(x1)) + x1
                    w = step_out(++q);
                    conv_sx_pair(c, rbk.c1[q - 1], rbk.c1[q], cur, T, w.raw, w.flags, (float)nk, S, /*chain=*/true);
                } else {
                    const void *in = fr ? static_cast<const void *>(cur) : static_cast<const void *>(cura);
                    // a step's closing conv: + x, the fp32 tensor or (rpl) recovered from the planes of the step's own input
                    // (a ResBlock2 step with the fp32 residual is given both slopes, as the upsampler)
                    SxOpt res = rbk.type1 || rpl ? act : lrelu;
                    res.div = (float)nk;
                    if (rpl) {
                        res.res_pl = cura;
                        res.res_slope = S;
                    } else
                        res.res = cur;
                    if (rbk.type1) {  // modules.py:301-314: x = c2(lrelu(c1(lrelu(x)))) + x  (tmp_raw and tmp_pl: one buffer)
                        conv_sx(c, rbk.c1[q], in, T, fr ? tmp_raw : nullptr, fr ? nullptr : tmp_pl, 0, act);
                        conv_sx(c, rbk.c2[q], tmp_pl, T, w.raw, w.pl, w.flags, res);
                    } else  // modules.py:355-364: x = c(lrelu(x)) + x
                        conv_sx(c, rbk.c1[q], in, T, w.raw, w.pl, w.flags, res);
                }
                cur = w.raw;
                cura = w.pl;
            }
        }
        // next stage input: the planes written by the final conv, or the raw x = xs / nk itself
        xa = (fr || last_stage) ? static_cast<const void *>(xs_raw) : static_cast<const void *>(xs_pl);
    }
    conv_post_sx(h, c, xs_raw, ylen, B, T, F, gb.out);
}

// The generator on the f32 engine: the only one for shapes the split-operand packing refuses.
void run_generator_f32(vits_handle *h, Ctx &c, const float *z, int64_t z_bstride, int z_cstride, const int *ylen, int B,
                       int F, const float *dec_cond, const GenBufs &gb) {
    const Model &m = h->model;
    hipStream_t st = h->stream;
    float *const *reg = gb.reg;
    // Every leaky_relu of the generator (models.py:354,364; modules.py:303,307,357) is applied by the
    // PRODUCER's epilogue, so no conv carries activation math in its MFMA loop (conv_engine.hip.hpp).
    // A tensor that is needed both raw (residual) and activated (next conv input) is stored twice.
    const float S = 0.1f;  // Generator.LRELU_SLOPE / ResBlock LRELU_SLOPE
    const int nst = (int)m.ups.size();
    ConvOpt gen;  // (no conv here has a prologue activation)
    gen.slope = 1.f;
    ConvOpt mid = gen;  // c1 of a ResBlock1 step: activated for c2
    mid.oslope = S;
    // xa = leaky_relu(conv_pre(z * y_mask) [+ cond(g)], 0.1)            (models.py:349-354)
    float *xa = reg[0];
    const int Fp = (F + 3) & ~3;  // pitch of conv_pre's output rows: lets ups[0] use the 16-byte DMA path
    ConvOpt pre = gen;
    pre.len = ylen;
    pre.bias_b = dec_cond;
    pre.bias_b_stride = m.C0;
    pre.oslope = S;
    pre.x_cstride = z_cstride;
    pre.out_cstride = Fp;
    conv(c, m.conv_pre, z, z_bstride, F, xa, (int64_t)m.C0 * Fp, ylen ? PRO_MASK : 0, pre);
    int T = F, Cc = m.C0, xs_idx = 0;
    int in_pitch = Fp;
    for (int si = 0; si < nst; si++) {
        const auto &stg = m.ups[si];
        // y = up(xa) as a pixel-shuffled dense conv; stored raw (residual) and activated (conv input)
        float *y = reg[2], *ya = reg[3];
        const int To = T * stg.u;
        ConvOpt up = gen;
        up.out2 = ya;
        up.oslope2 = S;
        up.x_cstride = in_pitch;
        conv(c, stg.up, xa, (int64_t)Cc * in_pitch, T, y, (int64_t)stg.C * To, 0, up);
        in_pitch = To;
        T = To;
        Cc = stg.C;
        const int64_t sCT = (int64_t)Cc * T;
        xs_idx ^= 1;
        float *xs = reg[xs_idx];
        float *ra[2] = {reg[4], reg[6]}, *raa[2] = {reg[5], reg[7]}, *tmp = reg[8];
        const int nk = (int)stg.rbs.size();
        // slope applied to the stage output: 0.1 before the next upsampler, 0.01 before conv_post (:364)
        const float out_slope = si == nst - 1 ? 0.01f : S;
        for (int j = 0; j < nk; j++) {
            const auto &rbk = stg.rbs[j];
            const float *cur = y, *cura = ya;
            for (int q = 0; q < rbk.n; q++) {
                // a step writes the block's stream raw and activated; the last one the running sum xs, which the final
                // block stores activated for its only consumer
                const bool last = q == rbk.n - 1;
                float *dst = last ? xs : ra[q & 1];
                const int fl = EPI_RES | (last ? mrf_flags(j, nk) : 0);
                ConvOpt res = gen;
                res.res = cur;
                res.res_bstride = sCT;
                res.div = (float)nk;
                res.oslope = last && j == nk - 1 ? out_slope : 1.f;
                res.out2 = last ? nullptr : raa[q & 1];
                res.oslope2 = S;
                if (rbk.type1) {  // modules.py:301-314: x = c2(lrelu(c1(lrelu(x)))) + x
                    conv(c, rbk.c1[q], cura, sCT, T, tmp, sCT, 0, mid);
                    conv(c, rbk.c2[q], tmp, sCT, T, dst, sCT, fl, res);
                } else  // modules.py:355-364: x = c(lrelu(x)) + x
                    conv(c, rbk.c1[q], cura, sCT, T, dst, sCT, fl, res);
                cur = dst;
                cura = res.out2;
            }
        }
        xa = xs;  // already activated for its only consumer
    }
    // conv_post; tanh (models.py:364-366): the leaky_relu(0.01) of models.py:364 was applied by the last stage's epilogue
    h->S = T;
    h->d_out = gb.out;  // (reg[9])
    launch_post_conv(st, B, m.post_cin, m.post_k, T, xa, c.P(m.post_w), h->d_out, 1.0f, tail_len(h, ylen), T / F);
    conv_post_account(h, c, B, T);
}

// One utterance batch through the generator: which walker a voice takes is decided here, once (Model::gen_sx: the
// split-operand packing took every conv; Model::gen_planes: its plane-stream form)
int run_generator(vits_handle *h, Ctx &c, const float *z, int64_t z_bstride, int z_cstride, const int *ylen, int B,
                  int F, const float *dec_cond, const GenBufs &gb) {
    const Model &m = h->model;
    h->cur_stage = 3;
    stage_mark(h, 3);
    if (!m.gen_sx) run_generator_f32(h, c, z, z_bstride, z_cstride, ylen, B, F, dec_cond, gb);
    else if (m.gen_planes) run_generator_planes(h, c, z, z_bstride, z_cstride, ylen, B, F, dec_cond, gb);
    else run_generator_sx(h, c, z, z_bstride, z_cstride, ylen, B, F, dec_cond, gb);
    c.rag = SxRagged{nullptr, 0, 0};
    stage_mark(h, 4);
    return 0;
}

__global__ void chunk_len_kernel(const int *ylen, int *out, int B, int lo, int n) {
    const int b = blockIdx.x * blockDim.x + threadIdx.x;
    if (b < B) {
        const int v = ylen ? ylen[b] - lo : n;  // (no lengths: every frame of the chunk is valid)
        out[b] = v < 0 ? 0 : (v > n ? n : v);
    }
}

// ---- output rate (vits_set_output_rate): the rendered waveform resampled on the device (resample.hip.hpp)

// the output samples of a row of S_in input samples, refused where a row does not admit them
int resample_count(vits_handle *h, int64_t S_in, int &S_out) {
    const ResamplePlan &p = h->rs.plan;
    const int64_t so = p.count(S_in);
    S_out = (int)so;
    if (so <= INT_MAX) return 0;
    return fail(h, VITS_E_ARG, "%lld samples at %d Hz are %lld samples at %d Hz: more than a row admits (%d)", (long long)S_in, p.fi,
                (long long)so, p.fo, INT_MAX);
}

// The staging slab carved for the resampled result of B rows of S_in input samples.  The run's inputs lived there: every
// kernel that read them precedes the resampler on the stream (and a growing slab waits for the stream first).
int resample_carve(vits_handle *h, int B, int64_t S_in, ResampleBufs &rb, int &S_out) {
    if (int rc = resample_count(h, S_in, S_out)) return rc;
    return slab_carve(h, h->io, "staging", [&](Carver &cv) { rb = carve_resample(cv, B, S_out, (int)h->rs.plan.K); });
}

// The whole waveform a run has just rendered (h->d_out, rows of h->S samples, ylen[b] * hop of them valid; no frame counts:
// all) -> [B][S_out] at the output rate.  d_out / S describe the resampled buffer afterwards.
int resample_run(vits_handle *h, const int *ylen, int B) {
    const ResamplePlan &p = h->rs.plan;
    const int S = h->S;
    ResampleBufs rb;
    int S_out = 0;
    if (int rc = resample_carve(h, B, S, rb, S_out)) return rc;
    hipStream_t st = h->stream;
    resample_counts_kernel<<<(B + 63) / 64, 64, 0, st>>>(ylen, h->model.hop, S, p.L, p.M, rb.n_in, rb.n_out, B);
    ResampleArgs a = resample_args(h->rs);
    a.x = h->d_out;
    a.x_pitch = S;
    a.x_n = S;
    a.n_in = rb.n_in;
    a.n_out = rb.n_out;
    a.y = rb.out;
    a.y_pitch = S_out;
    a.n_hi = S_out;
    const hipError_t e = launch_resample(a, B, /*piece=*/false, st);
    if (e != hipSuccess) return fail(h, VITS_E_DEVICE, "resampler launch failed: %s", hipGetErrorString(e));
    h->stats.total_launches += 2;
    h->d_out = rb.out;
    h->S = S_out;
    h->d_nout = rb.n_out;
    h->rs_run_K = (int)p.K;
    h->rs_run_L = p.L;
    h->rs_run_M = p.M;
    h->out_resampled = true;
    return 0;
}

// The same with a rate per row (vits_set_output_rates; B == the rows named, checked before the run began): [B][S_out],
// S_out = max_b N_b, through resample_rows_kernel.  The rows' counts are known on the host (h_ylen; no frame counts: all), so
// S_out is exact.  A run whose rows are all native launches nothing and leaves the native waveform where it is.
int resample_rows_run(vits_handle *h, const int *ylen, int B) {
    const auto &rw = h->rows;
    const int S = h->S;
    h->run_rates.assign(B, rw.fi);
    h->run_L.assign(B, 1);
    h->run_M.assign(B, 1);
    int64_t so = 1;
    int K = 0;
    for (int b = 0; b < B; b++) {
        int64_t n = ylen ? (int64_t)h->h_ylen[b] * h->model.hop : S;
        n = n < 0 ? 0 : (n > S ? S : n);
        if (rw.plan_of[b] >= 0) {
            const ResamplePlan &p = rw.plans[rw.plan_of[b]].plan;
            h->run_rates[b] = p.fo;
            h->run_L[b] = p.L;
            h->run_M[b] = p.M;
            K = p.K > K ? (int)p.K : K;
            n = p.count(n);
            if (n > INT_MAX) {
                forget_row_run(h);
                return fail(h, VITS_E_ARG, "row %d: its samples are %lld samples at %d Hz: more than a row admits (%d)", b, (long long)n, p.fo, INT_MAX);
            }
        }
        so = n > so ? n : so;
    }
    if (K == 0) return 0;  // every row native
    const int S_out = (int)so;
    ResampleBufs rb;
    if (int rc = slab_carve(h, h->io, "staging", [&](Carver &cv) { rb = carve_resample(cv, B, S_out, K); })) return rc;
    hipStream_t st = h->stream;
    resample_rows_counts_kernel<<<(B + 63) / 64, 64, 0, st>>>(ylen, h->model.hop, S, rw.d_recs, rb.n_in, rb.n_out, B);
    ResampleRowsArgs r{};
    r.plans = rw.d_recs;
    r.x = h->d_out;
    r.x_pitch = S;
    r.x_n = S;
    r.n_in = rb.n_in;
    r.n_out = rb.n_out;
    r.y = rb.out;
    r.y_pitch = S_out;
    r.n_hi = S_out;
    const hipError_t e = launch_resample_rows(r, B, rw.lds, st);
    if (e != hipSuccess) return fail(h, VITS_E_DEVICE, "resampler launch failed: %s", hipGetErrorString(e));
    h->stats.total_launches += 2;
    h->d_out = rb.out;
    h->S = S_out;
    h->d_nout = rb.n_out;
    h->rs_run_K = K;
    h->out_resampled = true;
    return 0;
}

// ---- intonation (vits_run_async_warped): the rendered waveform warped on the device (warp.hip.hpp)

// The whole waveform a run has just rendered (h->d_out, rows of h->S samples) -> [B][S_w], every token played back at its own
// speed.  The plans come from the host copy of the durations, which the run's one readback left: no synchronisation.
// d_out / S describe the warped buffer afterwards, as after resample_run.  (warp_run_planned, below.)

// the prototype table on the device (made by the first warped run) and the pinned block a plan is uploaded from
int warp_device_begin(vits_handle *h, size_t pin_bytes) {
    if (!h->warp_G) {
        std::vector<float> G(kWarpTable);
        warp_table(G.data());
        HIPCHECK(h, hipMalloc((void **)&h->warp_G, sizeof(float) * kWarpTable));
        HIPCHECK(h, hipMemcpy(h->warp_G, G.data(), sizeof(float) * kWarpTable, hipMemcpyHostToDevice));
    }
    // (the copies out of it that the previous run queued completed with this run's readback)
    if (h->warp_pin_cap < pin_bytes) {
        if (h->warp_pin) hipHostFree(h->warp_pin);
        h->warp_pin = nullptr;
        h->warp_pin_cap = 0;
        const size_t cap = pin_bytes < 65536 ? 65536 : pin_bytes + pin_bytes / 4;
        HIPCHECK(h, hipHostMalloc((void **)&h->warp_pin, cap));
        h->warp_pin_cap = cap;
    }
    return 0;
}

// The plans of a run's rows from the host copy of the durations, which the run's one readback left: no synchronisation.
// row_in: the input samples a row has at most.  The whole run (warp_run_planned) and the streamed one (render_chunks) plan
// HERE, through one of the two warp_plan_run below, chosen by the rows' type.  What they share: the durations must be the
// run's, a row's valid input is clamped to row_in, `plan` makes the records and S_w of it - "" or what is wrong -, and S_w
// must be a row's length.
template <class Plan>
int warp_plan_checked(vits_handle *h, int B, int T, int64_t row_in, int64_t &S_w, Plan plan) {
    if (h->h_dur_B != B || h->h_dur_T != T) return fail(h, VITS_E_ARG, "no durations to plan the warp from");
    std::vector<int64_t> n_in((size_t)B);
    for (int b = 0; b < B; b++) {
        const int64_t n = (int64_t)h->h_ylen[b] * h->model.hop;
        n_in[b] = n < 0 ? 0 : (n > row_in ? row_in : n);
    }
    const std::string e = plan(n_in);
    if (!e.empty()) return fail(h, VITS_E_ARG, "%s", e.c_str());
    if (S_w > INT_MAX) return fail(h, VITS_E_ARG, "a warped row of %lld samples: more than a row admits (%d)", (long long)S_w, INT_MAX);
    return 0;
}

// native rows: constant tokens plan with warp_plan, gliding ones (rr.semitones_end) with glide_plan
template <class Seg>
int warp_plan_run(vits_handle *h, const RunRows &rr, int B, int T, int64_t row_in, std::vector<Seg> &segs, std::vector<int32_t> &first,
                  std::vector<int64_t> &spans, std::vector<WarpRow> &rows, int64_t &S_w) {
    auto plan_row = [&](int b, const int64_t *dur, int len, int hp, Seg *sg, int64_t *sp, int64_t &ns, int64_t &N) -> std::string {
        const float *s0 = rr.semitones + (size_t)b * T;
        if constexpr (std::is_same_v<Seg, vits_warp_seg>) return warp_plan(dur, s0, len, hp, sg, sp, ns, N);
        else return glide_plan(dur, s0, rr.semitones_end + (size_t)b * T, len, hp, sg, sp, ns, N);
    };
    return warp_plan_checked(h, B, T, row_in, S_w, [&](const std::vector<int64_t> &n_in) {
        return warp_plan_rows(h->h_dur.data(), rr.semitone_lens, n_in.data(), B, T, h->model.hop, plan_row, segs, first, spans, rows, S_w);
    });
}

// ---- pitch at an output rate (vitsmi.h, "pitch at an output rate"): the rate folded into the warp's steps, one launch from the
// native waveform into the staging slab in place of resample_run / resample_rows_run + warp_run.

// the resampler's plan of row b under the handle's rate or the rows' rates (nullptr: a native row)
const ResampleDev *rate_of_row(const vits_handle *h, int b) {
    if (h->rs.plan.on()) return &h->rs;
    if (h->rows.on() && b < (int)h->rows.plan_of.size() && h->rows.plan_of[b] >= 0) return &h->rows.plans[h->rows.plan_of[b]];
    return nullptr;
}

// folded rows: an unpitched row leaves no record - it is an identity row, its spans the resampler's rule -; every other row is
// planned with its own (L_b, M_b) folded in
template <class Seg>
int warp_plan_run(vits_handle *h, const RunRows &rr, int B, int T, int64_t row_in, std::vector<Seg> &segs, std::vector<int32_t> &first,
                  std::vector<int64_t> &spans, std::vector<WarpRateRow> &rows, int64_t &S_w) {
    std::vector<int64_t> L((size_t)B, 1), M((size_t)B, 1);
    for (int b = 0; b < B; b++)
        if (const ResampleDev *d = rate_of_row(h, b)) {
            L[b] = d->plan.L;
            M[b] = d->plan.M;
        }
    const int rc = warp_plan_checked(h, B, T, row_in, S_w, [&](const std::vector<int64_t> &n_in) {
        auto plan_row = [&](int b, const int64_t *dur, int len, int hp, Seg *sg, int64_t *sp, int64_t &ns, int64_t &N) -> std::string {
            const float *s0 = rr.semitones + (size_t)b * T, *s1 = rr.semitones_end ? rr.semitones_end + (size_t)b * T : nullptr;
            if (warp_rate_unpitched(s0, s1, len)) {
                ns = 0;
                N = warp_rate_identity(dur, len, hp, L[b], M[b], n_in[b], sp);
                return "";
            }
            if constexpr (std::is_same_v<Seg, vits_warp_seg>) return warp_plan_rate(dur, s0, len, hp, L[b], M[b], sg, sp, ns, N);
            else return glide_plan_rate(dur, s0, s1, len, hp, L[b], M[b], sg, sp, ns, N);
        };
        std::vector<WarpRow> narrow;
        const std::string e = warp_plan_rows(h->h_dur.data(), rr.semitone_lens, n_in.data(), B, T, h->model.hop, plan_row, segs, first, spans, narrow, S_w);
        if (e.empty()) S_w = warp_rate_rows(segs.data(), first.data(), n_in.data(), L.data(), M.data(), B, rows);
        return e;
    });
    if (rc) return rc;
    for (int b = 0; b < B; b++)
        if (const ResampleDev *d = rate_of_row(h, b)) {
            rows[(size_t)b].table = d->table;
            rows[(size_t)b].Kp = d->Kp;
            rows[(size_t)b].K = (int32_t)d->plan.K;
        }
    return 0;
}

// what a warped run leaves for the host: the rows' output counts and k per token
template <class Row>
void warp_remember(vits_handle *h, const std::vector<Row> &rows, std::vector<int64_t> &&spans, int T) {
    h->warp_counts.resize(rows.size());
    for (size_t b = 0; b < rows.size(); b++) h->warp_counts[b] = rows[b].n_out;
    h->warp_spans = std::move(spans);
    h->warp_T = T;
}

// One body serves both record families (vits_glide_seg is a record of vits_warp_seg's size, so carve_warp carves either plan
// block) and both row widths: plan, carve, upload, the one launch, and what the run leaves - at the native rate.
template <class Seg, class Row>
int warp_run_planned(vits_handle *h, const RunRows &rr, int B, int T) {
    const int S = h->S;
    std::vector<Seg> segs;
    std::vector<int32_t> first;
    std::vector<int64_t> spans;
    std::vector<Row> rows;
    int64_t S_w = 1;
    if (int rc = warp_plan_run(h, rr, B, T, S, segs, first, spans, rows, S_w)) return rc;
    WarpBufs wb;
    if (int rc = slab_carve(h, h->io, "staging", [&](Carver &cv) { wb = carve_warp(cv, B, (int)S_w, (int64_t)segs.size(), sizeof(Row)); })) return rc;
    hipStream_t st = h->stream;
    // [segs | rows | n_out] in pinned memory
    if (int rc = warp_device_begin(h, wb.plan_bytes + (size_t)B * sizeof(int))) return rc;
    const size_t seg_bytes = segs.size() * sizeof(Seg);
    if (seg_bytes) std::memcpy(h->warp_pin, segs.data(), seg_bytes);
    std::memcpy(h->warp_pin + seg_bytes, rows.data(), (size_t)B * sizeof(Row));
    int *pin_nout = reinterpret_cast<int *>(h->warp_pin + wb.plan_bytes);
    for (int b = 0; b < B; b++) pin_nout[b] = rows[(size_t)b].n_out;
    HIPCHECK(h, hipMemcpyAsync(wb.segs, h->warp_pin, wb.plan_bytes, hipMemcpyHostToDevice, st));
    HIPCHECK(h, hipMemcpyAsync(wb.front.n_out, pin_nout, (size_t)B * sizeof(int), hipMemcpyHostToDevice, st));
    WarpArgsT<Seg, Row> a{};
    a.segs = reinterpret_cast<const Seg *>(wb.segs);
    a.rows = static_cast<const Row *>(wb.rows);
    a.G = h->warp_G;
    a.x = h->d_out;
    a.x_pitch = S;
    a.y = wb.front.out;
    a.y_pitch = S_w;
    a.n_hi = (int)S_w;
    const hipError_t e = launch_warp_tile(a, B, st);
    if (e != hipSuccess) return fail(h, VITS_E_DEVICE, "warp launch failed: %s", hipGetErrorString(e));
    h->stats.total_launches += 1;
    h->d_out = wb.front.out;
    h->S = (int)S_w;
    h->d_nout = wb.front.n_out;
    h->rs_run_K = 0;  // (carve_warp's walk: no carry)
    h->rs_run_L = h->rs_run_M = 1;
    h->out_resampled = true;
    warp_remember(h, rows, std::move(spans), T);
    return 0;
}

// constant tokens: warp_kernel; some token glides (rr.semitones_end): glide_kernel in its slot
int warp_run(vits_handle *h, const RunRows &rr, int B, int T) {
    return rr.semitones_end ? warp_run_planned<vits_glide_seg, WarpRow>(h, rr, B, T) : warp_run_planned<vits_warp_seg, WarpRow>(h, rr, B, T);
}

// ... at an output rate: the wide kernels, and what resample_run / resample_rows_run leave about the rates of a run
int warp_rate_run(vits_handle *h, const RunRows &rr, int B, int T) {
    if (int rc = rr.semitones_end ? warp_run_planned<vits_glide_seg, WarpRateRow>(h, rr, B, T) : warp_run_planned<vits_warp_seg, WarpRateRow>(h, rr, B, T))
        return rc;
    h->rs_run_L = h->rs.plan.on() ? h->rs.plan.L : 1;
    h->rs_run_M = h->rs.plan.on() ? h->rs.plan.M : 1;
    if (h->rows.on()) {
        h->run_rates.assign(B, h->rows.fi);
        h->run_L.assign(B, 1);
        h->run_M.assign(B, 1);
        for (int b = 0; b < B; b++)
            if (const ResampleDev *d = rate_of_row(h, b)) {
                h->run_rates[b] = d->plan.fo;
                h->run_L[b] = d->plan.L;
                h->run_M[b] = d->plan.M;
            }
    }
    return 0;
}

// The two pinned buffers (vits_handle::ring) finished pieces reach the host through.  A piece is copied into slot(); queue()
// records the slot's event, hands the piece queued before it to the caller - whose callback so runs while this one renders -
// and moves on to the other slot.  A piece that delivers nothing is never queued and the ring does not move: the pending slot,
// which the callback may still be reading, is never the next one written.
template <class Call>
struct ChunkRing {
    vits_handle *h;
    Call call;                          // the caller's callback over (slot, first, n): its answer
    int next = 0, pend = -1, stop = 0;  // stop: the last answer
    int64_t pend_first = 0, pend_n = 0;
    char *slot() const { return h->ring[next]; }
    int deliver() {  // hand the pending piece to the caller
        if (pend < 0) return 0;
        if (hipEventSynchronize(h->ring_ev[pend]) != hipSuccess) return fail(h, VITS_E_DEVICE, "chunk copy failed");
        stop = call(h->ring[pend], pend_first, pend_n);
        pend = -1;
        return 0;
    }
    int queue(int64_t first, int64_t n) {  // samples [first, first + n) of the rows have been enqueued into slot()
        HIPCHECK(h, hipEventRecord(h->ring_ev[next], h->stream));
        if (int rc = deliver()) return rc;  // (the previous piece, while this one renders)
        pend = next;
        pend_first = first;
        pend_n = n;
        next ^= 1;
        return 0;
    }
};

// Frames [0, F) of z rendered in chunks of sink->chunk_frames: each chunk is rendered together with gen_rf_frames of
// context on either side (clipped at the utterance ends, where the generator really sees zero padding) and only its
// interior is kept, so every sample equals the one an unchunked run produces (the convolutions accumulate in the same
// order wherever a column sits in a tile).  The interior then goes through the stages of stream_run.hip.hpp (resample, pack)
// and what is left to deliver reaches the host through the ring; the callback for chunk i runs while chunk i + 1 renders.
int render_chunks(vits_handle *h, Ctx &c, const float *z, int64_t z_bstride, int z_cstride, const int *ylen, int B, int F,
                  const float *dec_cond, const FrameBufs &fb, int Fgen, const ChunkSink &sink, const RunRows *pitch = nullptr, int T = 0) {
    const Model &m = h->model;
    hipStream_t st = h->stream;
    const int ov = m.gen_rf_frames, hop = m.hop;
    const int chunk = sink.chunk_frames;
    const ResamplePlan &rp = h->rs.plan;
    // an output rate: the batch path's [B][S_out], bit for bit - but a pitched stream folds the rate into the warp's steps
    // ("pitch at an output rate") and runs no resampler stage: the two are never both on
    const bool folded = pitch != nullptr && rp.on();
    const bool rs = rp.on() && !folded;
    const bool enc = sink.fmt != nullptr;  // the encoded form of the sink; false executes what it always executed
    // Streamed pitch (vitsmi.h, "streamed pitch"; at an output rate the folded plan: "pitch at an output rate"): the rows' plans first, from the
    // durations on the host - the whole run's planning -, so that everything below sees the OUTPUT timeline: S_w, N_b.
    const bool warp = pitch != nullptr;
    WarpRun wrun;
    int64_t cap_step = kWarpMinStep;  // what the cap of a delivery counts with: the plan's least step and (wrun.half) its largest Kh
    if (warp) {
        h->d_out = nullptr;  // (as under a plan callback: the run has begun, the host's counts are this run's from here on)
        wrun.glide = pitch->semitones_end != nullptr;
        wrun.folded = folded;
        const int rc = warp_run_visit(wrun, [&](auto &segs, auto &rows) {
            if (int rc = warp_plan_run(h, *pitch, B, T, (int64_t)F * hop, segs, wrun.first, wrun.spans, rows, wrun.S_w)) return rc;
            warp_remember(h, rows, std::vector<int64_t>(wrun.spans), T);
            warp_plan_extent(segs.data(), rows, wrun.half, cap_step);
            return 0;
        });
        if (rc) return rc;
    }
    // encoded form: the rows' valid samples (host: the callback's valid[]; device: the kernel's)
    std::vector<int64_t> row_n;
    if (enc) {
        row_n.resize((size_t)B);
        for (int b = 0; b < B; b++) {
            const int64_t nb = (int64_t)(ylen ? h->h_ylen[b] : F) * hop;
            row_n[b] = warp ? (int64_t)wrun.row_out(b) : rs ? rp.count(nb) : nb;
        }
    }
    // The shaped form of the encoded sink (vitsmi.h, "shaped streaming"): the plan callback first - the durations and the
    // rows' sample counts are on the host, nothing of this run's audio exists yet -, then what it wrote through the checks of
    // up-front shaping.  Without fades, points and look-ahead everything below is the unshaped stream's.
    vits_stream_shaping shp{};
    bool shaped = false;
    if (enc && stream_shaped(sink.shaping, B)) {
        shp = *sink.shaping;
        if (shp.plan) {
            // (the run has begun: whatever the callback answers, the previous run's waveform no longer belongs to the frame
            // counts and durations on the host - a refusal below leaves "no completed run")
            h->d_out = nullptr;
            const bool tokens = ylen != nullptr && h->h_dur_B == B && h->h_dur_T > 0;
            const int T = tokens ? h->h_dur_T : 0;
            std::vector<int64_t> dur((size_t)B * T);
            for (size_t i = 0; i < dur.size(); i++) dur[i] = (int64_t)h->h_dur[i];
            if (shp.plan(shp.plan_user, B, T, tokens ? dur.data() : nullptr, row_n.data(), &shp) != 0)
                return fail(h, VITS_E_ARG, "the stream's plan callback refused the run");
            if (shp.lookahead != sink.shaping->lookahead)
                return fail(h, VITS_E_ARG, "the stream's plan callback changed lookahead from %d to %d", sink.shaping->lookahead, shp.lookahead);
            const std::string e = stream_shape_fault(&shp, sink.fmt->volume, B);
            if (!e.empty()) return fail(h, VITS_E_ARG, "plan callback: %s", e.c_str());
        }
        shaped = shp.lookahead > 0 || any_shape(shp.shapes, B);
    }
    // The trimmed form (vitsmi.h, "trimmed streaming"): the onsets are the call's - the plan callback has no say in them - and a
    // trimmed stream takes the shaped kernels, with an empty shaping where there is none.
    const bool trimmed = enc && stream_trimmed(sink.onsets, B);
    shaped = shaped || trimmed;
    // the sizes of the run's pieces, the one walk of the staging slab, the ring
    const int sL = shaped ? shp.lookahead : 0;  // the last chunk delivers sL samples more than it renders
    int S_out = 0;
    if (rs)
        if (int rc = resample_count(h, (int64_t)F * hop, S_out)) return rc;
    const int64_t n_cap = warp ? warp_stream_cap((int64_t)(chunk < F ? chunk : F) * hop, wrun.S_w, cap_step, wrun.half) : 0;
    const int64_t total = warp ? wrun.S_w : rs ? (int64_t)S_out : (int64_t)F * hop;
    const int64_t n_max = warp ? (n_cap + sL < total ? n_cap + sL : total) : stream_n_max(rp, chunk, F, hop, sL, total);
    StreamBufs sb{};
    WarpStreamBufs wsb{};
    if (int rc = slab_carve(h, h->io, "staging", [&](Carver &cv) {
            if (warp) wsb = carve_warp_stream(cv, B, (int64_t)F * hop, n_cap, wrun.n_segs(), wrun.row_bytes());
            sb = carve_stream(cv, B, total, n_max, rs ? (int)rp.K : 0, enc, shaped, sL, shaped ? stream_knot_count(&shp, B) : 0, trimmed);
        }))
        return rc;
    if (warp) {
        if (int rc = warp_device_begin(h, wsb.plan_bytes + (size_t)B * sizeof(int))) return rc;
        HIPCHECK(h, warp_run_begin(wrun, wsb, h->warp_G, n_cap, B, h->warp_pin, st));
    }
    ResampleRun rrun;
    if (rs) {
        HIPCHECK(h, resample_run_begin(rrun, h->rs, sb.rs, ylen, hop, F * hop, S_out, B, st));
        h->stats.total_launches++;
    }
    const size_t ring_bytes = stream_ring_bytes(B, n_max, enc ? delivery_width(sink.fmt->encoding) : 0, trimmed);
    if (ring_bytes > h->ring_cap) {
        for (auto &r : h->ring) {
            if (r) hipHostFree(r);
            r = nullptr;
        }
        h->ring_cap = 0;
        for (auto &r : h->ring)
            if (hipHostMalloc((void **)&r, ring_bytes) != hipSuccess) return fail(h, VITS_E_NOMEM, "pinned chunk buffer (%zu bytes)", ring_bytes);
        h->ring_cap = ring_bytes;
    }
    for (auto &e : h->ring_ev)
        if (!e) hipEventCreateWithFlags(&e, hipEventDisableTiming);
    StreamPackRun prun;
    if (enc)
        HIPCHECK(h, stream_pack_begin(prun, sink.fmt, shaped ? &shp : nullptr, B, sb.sp, sb.ss,
                                      warp ? StreamPackRows{wsb.n_out, 1, (int)total}
                                      : rs ? StreamPackRows{sb.rs.n_out, 1, S_out}
                                           : StreamPackRows{ylen, hop, F * hop},
                                      total, st,
                                      trimmed ? sink.onsets : nullptr, row_n.data()));
    std::vector<int32_t> valid((size_t)(enc ? B : 0)), skip((size_t)(enc ? B : 0), 0);
    auto call = [&](const char *buf, int64_t first, int64_t n) -> int {  // the caller's callback over a finished piece
        if (!enc) return sink.fn ? sink.fn(sink.user, reinterpret_cast<const float *>(buf), B, first, n, total) : 0;
        const int64_t pitch = (int64_t)StreamPackBufs::pitch(prun.width, n);
        for (int b = 0; b < B; b++) valid[b] = (int32_t)std::clamp<int64_t>(row_n[b] - first, 0, n);
        const float *peaks = reinterpret_cast<const float *>(buf + (size_t)B * pitch);
        if (trimmed) {  // the rows' starts came with the peaks: the skips, and whether the next piece is still scanned
            const int32_t *start = reinterpret_cast<const int32_t *>(peaks + StreamPackBufs::peak_floats(B));
            for (int b = 0; b < B; b++) skip[b] = (int32_t)std::clamp<int64_t>((int64_t)start[b] - first, 0, valid[b]);
            stream_pack_seen(prun, start, first + n, B);
        }
        if (sink.tfn) return sink.tfn(sink.user, buf, B, pitch, first, n, valid.data(), skip.data(), peaks, total);
        return sink.efn ? sink.efn(sink.user, buf, B, pitch, first, n, valid.data(), peaks, total) : 0;
    };
    ChunkRing<decltype(call)> ring{h, call};
    // What is left of a piece behind the stages in front - x [B][pn] at `first` (dense: its pitch is pn) - through the pack stage
    // into the ring.
    auto hand_over = [&](const float *x, int64_t x_pitch, int64_t first, int64_t pn, bool dense) -> int {
        int launches = 0;
        unsigned char *d = nullptr;
        size_t pitch = 0;
        if (enc && pn > 0) {
            const hipError_t e = stream_pack_piece(prun, x, x_pitch, first, pn, B, st, d, first, pn, pitch, launches);
            if (e != hipSuccess) return fail(h, VITS_E_DEVICE, "%sstream pack launch failed: %s", shaped ? "shaped " : "", hipGetErrorString(e));
            h->stats.total_launches += launches;
        }
        // (a chunk shorter than the filter's or the limiter's look-ahead completes nothing: no copy, no call, the same slot next)
        if (pn <= 0) return 0;
        if (enc)  // bytes and peaks - a trimmed stream: and starts - in one copy
            HIPCHECK(h, hipMemcpyAsync(ring.slot(), d, (size_t)B * pitch + prun.tail_bytes(B), hipMemcpyDeviceToHost, st));
        else if (dense)
            HIPCHECK(h, hipMemcpyAsync(ring.slot(), x, (size_t)B * pn * 4, hipMemcpyDeviceToHost, st));
        else  // straight out of the rendered rows
            HIPCHECK(h, hipMemcpy2DAsync(ring.slot(), (size_t)pn * 4, x, (size_t)x_pitch * 4, (size_t)pn * 4, B, hipMemcpyDeviceToHost, st));
        return ring.queue(first, pn);
    };
    // per-chunk valid lengths, ALWAYS passed: a chunk is a window into rows whose neighbours are real data, and only a
    // length mask makes the conv engines bound their reads by the chunk instead of by the row pitch
    int *yl = fb.gen.yl;
    Carver cv(h->frm.base, h->frm.cap);
    const int *const whole_len = c.h_len;  // host copy of ylen (or nullptr)
    for (int f0 = 0; f0 < F && !ring.stop; f0 += chunk) {
        const int f1 = f0 + chunk < F ? f0 + chunk : F;
        const int lo = f0 - ov > 0 ? f0 - ov : 0, hi = f1 + ov < F ? f1 + ov : F, n = hi - lo;
        cv.rewind(fb.gen_at);  // the previous chunk's workspace (its copy-out precedes this chunk on the stream)
        const GenBufs gb = carve_generator(cv, m, B, Fgen);
        chunk_len_kernel<<<(B + 63) / 64, 64, 0, st>>>(ylen, yl, B, lo, n);
        // (host mirror of chunk_len_kernel for the ragged accounting; without frame counts every frame is valid)
        std::vector<int> hyl((size_t)B, n);
        if (ylen && whole_len)
            for (int b = 0; b < B; b++) hyl[b] = whole_len[b] - lo < 0 ? 0 : (whole_len[b] - lo > n ? n : whole_len[b] - lo);
        c.h_len = ylen && !whole_len ? nullptr : hyl.data();
        const int rc_gen = run_generator(h, c, z + lo, z_bstride, z_cstride, yl, B, n, dec_cond, gb);
        c.h_len = whole_len;
        if (rc_gen) return rc_gen;
        if (c.err != hipSuccess) return fail(h, VITS_E_DEVICE, "kernel launch failed: %s", hipGetErrorString(c.err));
        // the piece: the chunk's interior, samples [first, first + pn) of every row at x - what each stage leaves of it
        const float *x = h->d_out + (int64_t)(f0 - lo) * hop;
        int64_t x_pitch = h->S, first = (int64_t)f0 * hop, pn = (int64_t)(f1 - f0) * hop;
        int launches = 0;
        if (rs) {
            const hipError_t e = resample_run_piece(rrun, x, x_pitch, first, pn, f1 == F, B, st, first, pn, launches);
            if (e != hipSuccess) return fail(h, VITS_E_DEVICE, "resampler launch failed: %s", hipGetErrorString(e));
            h->stats.total_launches += launches;
            x = sb.rs.out;  // [B][pn]
            x_pitch = pn;
        }
        if (warp) {  // the history takes the piece; what that completes goes on in windows of at most n_cap output samples
            const hipError_t ew = warp_run_piece(wrun, x, x_pitch, first, pn, f1 == F, B, st);
            if (ew != hipSuccess) return fail(h, VITS_E_DEVICE, "warp history copy failed: %s", hipGetErrorString(ew));
            while (!ring.stop) {
                const hipError_t e = warp_run_window(wrun, B, st, x, first, pn, launches);
                if (e != hipSuccess) return fail(h, VITS_E_DEVICE, "warp launch failed: %s", hipGetErrorString(e));
                if (pn <= 0) break;
                h->stats.total_launches += launches;
                if (int rc = hand_over(x, pn, first, pn, /*packed_rows=*/true)) return rc;
            }
            continue;
        }
        if (int rc = hand_over(x, x_pitch, first, pn, rs)) return rc;
    }
    if (!ring.stop)
        if (int rc = ring.deliver()) return rc;
    h->S = (int)total;
    h->d_out = nullptr;  // (no whole waveform exists on the device after a chunked run)
    return 0;
}

int run_frames(vits_handle *h, int B, int T, const RunRows &rr, const int64_t *d_sid, const float *d_noise_z,
               int64_t noise_z_stride, uint64_t seed, const ChunkSink *sink = nullptr) {
    const Model &m = h->model;
    const int C = m.C, Freal = h->F, Hf = m.flow_H;
    if (d_noise_z && noise_z_stride < Freal)
        return fail(h, VITS_E_ARG, "noise_z has %lld frames per row but %d are needed", (long long)noise_z_stride, Freal);
    // The flow runs on F rounded up to a multiple of 4 frames: every tensor in it is masked by y_len, so the
    // extra (masked) frames change nothing, and all its rows become 16-byte aligned for the conv engine's
    // 16-byte LDS-DMA.  The generator, which is NOT masked, runs on exactly Freal frames and reads z through
    // its row pitch.
    const int F = (Freal + 3) & ~3;
    h->Fpitch = F;
    const size_t nCF = (size_t)B * C * F;
    const int Fgen = gen_frames(m, F, sink ? sink->chunk_frames : 0);
    FrameBufs fb;
    if (int rc = slab_carve(h, h->frm, "frame", [&](Carver &cv) { fb = carve_frames(cv, m, B, F, Fgen, /*flow=*/true); })) return rc;
    const FlowBufs &w = fb.flow;
    Ctx c{h, m, h->stream, h->arena_dev, B};
    if ((int)h->h_ylen.size() == B) c.h_len = h->h_ylen.data();
    hipStream_t st = h->stream;
    const int *len = h->d_len, *ylen = h->d_ylen;
    float *zp = w.zp, *z = w.z;
    h->d_zp = zp;
    h->d_z = z;
    h->cur_stage = 2;
    stage_mark(h, 2);
    {
        // Ragged flow: only when EVERY launch of the flow is a conv_sx() launch (pre / gated in-layer / res_skip / post on the
        // split-operand engine: every f16x3 voice) - a kernel without the per-utterance end would read what its predecessor
        // did not write.  Masked either way, so results are those of the padded form, bit for bit.
        static const bool off = std::getenv("VITSMI_NO_RAGGED_FLOW") != nullptr;  // A/B timing
        bool all_sx = !off && B > 1 && c.h_len && (C / 2) % 32 == 0 && Hf % 32 == 0;
        for (const auto &cd : m.flow) {
            all_sx = all_sx && cd.pre_sx.sx && cd.post_sx.sx && cd.n_wn > 0;
            for (int i = 0; i < cd.n_wn && all_sx; i++)
                all_sx = cd.wn[i].in.sx && cd.wn[i].in.f16 && cd.wn[i].in.gate && cd.wn[i].rs_sx.sx;
        }
        if (all_sx) {
            double fr = 0;
            for (int b = 0; b < B; b++) fr += c.h_len[b] < F ? c.h_len[b] : F;
            c.flow_len = ylen;
            c.flow_frac = fr / ((double)B * F);
        }
    }
    const float noise_scale = rr.at(0, 0);
    const float *nz = nullptr;
    int64_t nzs = F;
    if (rr.any(B, 0)) {
        if (d_noise_z) {
            nz = d_noise_z;
            nzs = noise_z_stride;
        } else if (!rr.d_seeds) {
            float *g = w.g;
            launch_fill_normal(st, g, (int64_t)nCF, seed, 2);
            h->stats.total_launches++;
            nz = g;
        }
    }
    // m_p / logs_p are the two halves of the proj output: channel stride T, batch stride 2*C*T
    // (with per-utterance seeds and no injected noise, the kernel draws each utterance's prior noise itself)
    launch_expand_prior(st, B, C, T, F, h->d_mp, h->d_logs, (int64_t)2 * C * T, h->d_cum, len, ylen, nz, nzs, noise_scale,
                        rr.d_rows, nz ? nullptr : rr.d_seeds, zp, nz == d_noise_z ? Freal : F);
    h->stats.total_launches++;
    if (c.flow_len) {
        // z = z_p * y_mask: the ragged flow leaves the frames behind an utterance's end alone, where the reference's couplings
        // zero them one half at a time ((x1 - m) * mask, modules.py:464) - same z wherever it is valid, and the zeros the
        // reference ends up with behind
        masked_copy_kernel<<<dim3((F + 255) / 256, C, B), 256, 0, st>>>(zp, z, ylen, C, F);
        h->stats.total_launches++;
    } else
        HIPCHECK(h, hipMemcpyAsync(z, zp, nCF * 4, hipMemcpyDeviceToDevice, st));

    // ---- inverse coupling flow (models.py:247-254, modules.py:447-466); Flips folded at pack time
    float *hx = w.hx, *skip = w.skip, *acts = w.acts, *a2 = w.a2;
    uint16_t *hx_pl = w.hx_pl;  // planes of hx (sx in-layers)
    const int half = C / 2;
    const int64_t sCF = (int64_t)C * F, sHF = (int64_t)Hf * F;
    uint16_t *acts_pl = reinterpret_cast<uint16_t *>(a2);  // (a2 is unused where the gate writes operand planes)
    // pre / post on the split-operand engine (CouplingDesc::pre_sx): planes of x0 (written by the previous coupling's post:
    // its x1 is this one's x0; split here for the first) and of the skip sum (written by the last res_skip conv)
    uint16_t *x0_pl = w.x0_pl, *skip_pl = w.skip_pl;
    bool x0_planes_ready = false;
    ConvOpt masked;  // the convs whose flags mask by the frame counts
    masked.len = ylen;
    SxOpt masked_sx;
    masked_sx.len = ylen;
    for (size_t ci = 0; ci < m.flow.size(); ci++) {
        const auto &cd = m.flow[ci];
        const bool pp = cd.pre_sx.sx && cd.post_sx.sx && half % 32 == 0;
        const bool pp_next = ci + 1 < m.flow.size() && m.flow[ci + 1].pre_sx.sx && m.flow[ci + 1].post_sx.sx;
        float *gc = nullptr;
        const int gc_rows = 2 * Hf * cd.n_wn;
        if (m.gin) {
            gc = w.gc[ci];
            cond_matvec_kernel<<<dim3((gc_rows + 63) / 64, B), 64, 0, st>>>(c.P(m.emb_g), d_sid, m.n_speakers, c.P(cd.cond_w),
                                                                           c.P(cd.cond_b), gc, gc_rows, m.gin);
            h->stats.total_launches++;
        }
        const float *x0 = z + (cd.swapped ? (int64_t)half * F : 0);
        float *x1 = z + (cd.swapped ? 0 : (int64_t)half * F);
        // Launches per WN layer: [in-layer conv on the split engine] [tanh * sigmoid gate] [res_skip 1x1 conv].  The
        // res_skip conv's epilogue applies the update (x = (x + res) * mask, skip += ...: EPI_WN) and, when the next
        // in-layer runs on the split engine, also emits x as that conv's fp16 operand planes - as `pre` does for the
        // first layer - so neither an update nor a split launch is left (they were 2 of the 5 launches of a layer).
        const bool planes0 = cd.n_wn > 0 && cd.wn[0].in.sx && cd.wn[0].in.f16 && Hf % 32 == 0;
        ConvOpt pre = masked;
        pre.out_pl = planes0 ? hx_pl : nullptr;
        pre.pl_rows = Hf;
        // h = pre(x0) * mask
        if (pp) {
            if (!x0_planes_ready) {
                sx_split_planes_kernel<<<dim3((F + 255) / 256, half / 8, B), 256, 0, st>>>(x0, sCF, F, nullptr, x0_pl, half, F, 1,
                                                                                        range_slots(h, true));
                h->stats.total_launches++;
            }
            conv_sx_planar(c, cd.pre_sx, x0_pl, F, hx, planes0 ? hx_pl : nullptr, EPI_MASK, masked_sx);
        } else
            conv(c, cd.pre, x0, sCF, F, hx, sHF, EPI_MASK, pre);
        x0_planes_ready = false;
        for (int i = 0; i < cd.n_wn; i++) {
            const bool last = i == cd.n_wn - 1;
            const float *gc_i = gc ? gc + (int64_t)i * 2 * Hf : nullptr;  // the layer's rows of the speaker conditioning
            // x_in = in_layer(h) + g_l ; acts = tanh * sigmoid ; rs = res_skip(acts)
            if (cd.wn[i].in.sx) {
                SxOpt gcond;
                gcond.bias_b = gc_i;
                gcond.bias_b_stride = gc_rows;
                // split-operand engine: planes of hx (from the producing epilogue, or split here), conv to the raw cell
                // layout, gate reads that layout
                const bool have_planes = cd.wn[i].in.f16 && Hf % 32 == 0;
                if (!have_planes) {
                    sx_split_planes_kernel<<<dim3((F + 255) / 256, Hf / 8, B), 256, 0, st>>>(hx, sHF, F, nullptr, hx_pl, Hf, F,
                                                                                             cd.wn[i].in.f16 ? 1 : 0,
                                                                                             range_slots(h, cd.wn[i].in.f16));
                    h->stats.total_launches++;
                }
                if (cd.wn[i].in.gate && cd.wn[i].rs_sx.sx) {
                    // gate in the in-layer's epilogue, acts handed over as fp16 operand planes; the res_skip 1 x 1 conv on
                    // the same engine reads them and folds the update in: x += res * mask (+ the next in-layer's planes),
                    // skip += .. (the first layer stores it)
                    conv_sx(c, cd.wn[i].in, hx_pl, F, nullptr, acts_pl, SX_GATE, gcond);
                    SxOpt w = masked_sx;
                    w.out_raw2 = skip;
                    w.row_split = last ? 0 : Hf;
                    const bool np = !last && cd.wn[i + 1].in.sx && cd.wn[i + 1].in.f16 && Hf % 32 == 0;
                    w.pl_rows = np ? Hf : 0;
                    uint16_t *rs_pl = np ? hx_pl : nullptr;
                    if (last && pp) {  // the finished skip sum as post's operand planes
                        w.pl_rows = Hf;
                        w.pl_of2 = true;
                        rs_pl = skip_pl;
                    }
                    // (the first layer stores its skip rows: no zero fill of skip, no read of it)
                    conv_sx(c, cd.wn[i].rs_sx, acts_pl, F, hx, rs_pl, SX_WN_RMW | EPI_ACC | EPI_MASK | (i == 0 ? SX_PLANAR_STORE2 : 0), w);
                    continue;
                } else if (cd.wn[i].in.gate) {  // tanh * sigmoid in the conv's epilogue: acts directly
                    conv_sx(c, cd.wn[i].in, hx_pl, F, acts, nullptr, SX_GATE, gcond);
                    h->stats.total_launches--;  // (no gate launch: undo the increment below)
                } else {
                    conv_sx(c, cd.wn[i].in, hx_pl, F, a2, nullptr, 0, gcond);
                    wn_gate_blocked_kernel<<<dim3((F + 255) / 256, Hf / 8, B), 256, 0, st>>>(a2, acts, Hf, F);
                }
            } else {
                ConvOpt gcond;
                gcond.bias_b = gc_i;
                gcond.bias_b_stride = gc_rows;
                conv(c, cd.wn[i].in, hx, sHF, F, a2, 2 * sHF, 0, gcond);
                wn_gate_kernel<<<dim3((F + 255) / 256, Hf, B), 256, 0, st>>>(a2, acts, Hf, F);
            }
            h->stats.total_launches++;
            // res_skip conv + update: rows [0, Hf) -> hx (residual half), rows [Hf, 2 Hf) -> skip; last layer: skip only
            ConvOpt upd = masked;
            upd.out2 = skip;
            upd.wn_split = last ? 0 : Hf;
            const bool next_planes = !last && cd.wn[i + 1].in.sx && cd.wn[i + 1].in.f16 && Hf % 32 == 0;
            upd.out_pl = next_planes ? hx_pl : nullptr;
            upd.pl_rows = Hf;
            conv(c, cd.wn[i].rs, acts, sHF, F, hx, sHF, EPI_WN | EPI_MASK | (i == 0 ? EPI_WN_FIRST : 0), upd);
        }
        // x1 = (x1 - post(skip)*mask) * mask
        if (pp) {
            SxOpt w = masked_sx;
            w.row_split = half;
            w.planar_bstride = sCF;           // (x1's rows live inside z)
            w.pl_rows = pp_next ? half : 0;   // ... and are the next coupling's x0: its operand planes
            conv_sx(c, cd.post_sx, skip_pl, F, x1, pp_next ? x0_pl : nullptr, SX_WN_RMW | EPI_ACC | EPI_MASK | SX_PLANAR_COUPLING, w);
            x0_planes_ready = pp_next;
        } else
            conv(c, cd.post, skip, sHF, F, x1, sCF, EPI_COUPLING, masked);
    }
    c.note(hipGetLastError());

    float *dec_cond = nullptr;
    if (m.gin) {
        dec_cond = w.dec_cond;
        cond_matvec_kernel<<<dim3((m.C0 + 63) / 64, B), 64, 0, st>>>(c.P(m.emb_g), d_sid, m.n_speakers, c.P(m.dec_cond_w),
                                                                    c.P(m.dec_cond_b), dec_cond, m.C0, m.gin);
        h->stats.total_launches++;
    }
    if (sink) return render_chunks(h, c, z, sCF, F, ylen, B, Freal, dec_cond, fb, Fgen, *sink, rr.semitones ? &rr : nullptr, T);
    if (int rc = run_generator(h, c, z, sCF, F, ylen, B, Freal, dec_cond, fb.gen)) return rc;
    if (c.err != hipSuccess) return fail(h, VITS_E_DEVICE, "kernel launch failed: %s", hipGetErrorString(c.err));
    return 0;
}

}  // namespace

// ================================================================================== C ABI

// precision: an explicit arithmetic name (vits_open_opts), or nullptr = VITSMI_GEN_PRECISION / the default
static int open_common(const char *path, vits_handle **out, bool host_only, int device, void *ext_arena,
                       size_t ext_bytes, bool layout_only = false, const char *precision = nullptr) {
    if (!out || !path) return fail(nullptr, VITS_E_ARG, "null argument");
    *out = nullptr;
    OnnxModel om;
    std::string e = om.load(path);
    if (!e.empty()) return fail(nullptr, e.rfind("cannot open", 0) == 0 ? VITS_E_IO : VITS_E_FORMAT, "%s", e.c_str());
    vits_handle *h = new vits_handle();
    // a handle that adopts a resident arena only needs the layout (offsets, descriptors): no weight is re-packed
    e = h->model.build(om, /*layout_only=*/ext_arena != nullptr || layout_only, precision);
    if (!e.empty()) {
        delete h;
        return fail(nullptr, VITS_E_FORMAT, "%s: %s", path, e.c_str());
    }
    if (h->model.window > 4) {
        const int window = h->model.window;  // (read before the handle goes: the message once named a freed handle's field)
        delete h;
        return fail(nullptr, VITS_E_FORMAT, "attention window %d > 4 is unsupported", window);
    }
    // (the widest attention instantiation, DKB = 4, covers 128 channels per head: a wider head would lose channels 128.. from
    // its scores and leave their output rows unwritten)
    if (h->model.dk > kAttMaxHeadWidth) {
        const int dk = h->model.dk;
        delete h;
        return fail(nullptr, VITS_E_FORMAT, "attention head width %d > %d is unsupported", dk, kAttMaxHeadWidth);
    }
    h->host_only = host_only;
    {
        const char *te = std::getenv("VITSMI_TAILS");  // "reference": the graph's padded rendering (see vits_set_tails)
        h->tails_reference = te && std::string(te) == "reference";
    }
    {
        // Arithmetic of the generator's convs on the split-exact engine (fp32 operands and results in every mode):
        //   f16x3  (default) two fp16 planes per operand, three MFMA products: each product within ~3 * 2^-24
        //   bf16x6 three bf16 planes, six products: each product exact to 2^-24
        //   f16    the reduced-precision vocoder of BASELINE config 4: ONE fp16 plane per operand, one product, fp32
        //          accumulation, generator activations stored as fp16 (everything in front of z unchanged)
        // gen_nprod: 2 = f16x3, 1 = f16 (Model::build packed the weights for either), 6 = the six bf16 plane products.
        const Model::Precision pr = h->model.precision;  // (resolved by Model::build, which refuses an unknown name)
        h->gen_nprod = pr == Model::Precision::F16X3 ? 2 : (pr == Model::Precision::F16 ? 1 : 6);
        if (!h->model.gen_sx) {
            // (a generator the split-operand engine cannot take - a channel count that is not a multiple of 32 - runs on the f32
            // engine: fine for the two fp32-grade requests, whose results it matches, but NOT a reduced-precision vocoder: an
            // explicit "f16" request is refused with the reason, as a conv that fails the single-plane constraints already is)
            if (h->gen_nprod == 1) {
                delete h;
                return fail(nullptr, VITS_E_ARG, "gen_precision \"f16\" needs a generator on the split-operand engine (every channel "
                                                 "count a multiple of 32); this voice's runs on the f32 engine");
            }
            h->gen_nprod = 6;
        }
    }
    if (!host_only) {
        int n = 0;
        hipError_t er = hipGetDeviceCount(&n);
        if (er != hipSuccess || device < 0 || device >= n) {
            delete h;
            return fail(nullptr, VITS_E_DEVICE, "no usable HIP device %d (count %d): %s", device, n,
                        er == hipSuccess ? "index out of range" : hipGetErrorString(er));
        }
        h->device = device;
        if (hipSetDevice(device) != hipSuccess || hipStreamCreateWithFlags(&h->stream, hipStreamNonBlocking) != hipSuccess) {
            delete h;
            return fail(nullptr, VITS_E_DEVICE, "cannot create stream on device %d", device);
        }
        size_t bytes = (size_t)h->model.arena_floats * 4;
        if (ext_arena) {
            if (ext_bytes != bytes) {
                delete h;
                return fail(nullptr, VITS_E_ARG, "arena size mismatch: got %zu, model needs %zu", ext_bytes, bytes);
            }
            h->arena_dev = (float *)ext_arena;
        } else {
            if (hipMalloc((void **)&h->arena_dev, bytes) != hipSuccess ||
                hipMemcpy(h->arena_dev, h->model.arena.data(), bytes, hipMemcpyHostToDevice) != hipSuccess) {
                delete h;
                return fail(nullptr, VITS_E_NOMEM, "cannot place %zu-byte weight arena on device %d", bytes, device);
            }
            h->arena_owned = true;
        }
        for (auto &e2 : h->ev) hipEventCreate(&e2);
        if (!std::getenv("VITSMI_NO_RANGE_GUARD")) {  // range guard of the fp16 operand planes (generator, flow WN convs);
                                                     // the switch exists for A/B timing of its cost only
            const size_t nb = (size_t)kMaxRangeLaunches * kSxPeakSlots * kSxPeakStride * sizeof(unsigned);
            if (hipMalloc((void **)&h->d_range, nb + 64) != hipSuccess || hipHostMalloc((void **)&h->h_range, 64) != hipSuccess) {
                vits_close(h);
                return fail(nullptr, VITS_E_NOMEM, "cannot allocate the range-guard buffers");
            }
            h->d_range_res = reinterpret_cast<float *>(reinterpret_cast<char *>(h->d_range) + nb);
            hipMemset(h->d_range, 0, nb + 64);
            std::memset(h->h_range, 0, 64);
        }
    }
    *out = h;
    return VITS_OK;
}

extern "C" {

int vits_open(const char *p, int dev, vits_handle **out) { return open_common(p, out, false, dev, nullptr, 0); }
int vits_open_with_arena(const char *p, int dev, void *arena, size_t bytes, vits_handle **out) {
    if (!arena) return fail(nullptr, VITS_E_ARG, "null arena");
    return open_common(p, out, false, dev, arena, bytes);
}
int vits_open_host(const char *p, vits_handle **out) { return open_common(p, out, true, -1, nullptr, 0); }
int vits_open_layout(const char *p, vits_handle **out) { return open_common(p, out, true, -1, nullptr, 0, true); }

int vits_open_opts(const char *p, const vits_open_options *o, vits_handle **out) {
    if (!o) return fail(nullptr, VITS_E_ARG, "null options");
    if (o->arena_dev && o->host_only) return fail(nullptr, VITS_E_ARG, "host_only excludes arena_dev");
    return open_common(p, out, o->host_only != 0, o->host_only ? -1 : o->device_id, o->arena_dev, o->arena_bytes,
                       o->layout_only != 0, o->gen_precision);
}

static void row_rates_drop(vits_handle *h, const vits_handle::RowRates *keep = nullptr);

void vits_close(vits_handle *h) {
    if (!h) return;
    if (!h->host_only) {
        hipSetDevice(h->device);
        if (h->stream) hipStreamSynchronize(h->stream);
        if (h->arena_owned && h->arena_dev) hipFree(h->arena_dev);
        if (h->h_rb_pin) hipHostFree(h->h_rb_pin);
        if (h->h_in_pin) hipHostFree(h->h_in_pin);
        if (h->tok.base) hipFree(h->tok.base);
        if (h->frm.base) hipFree(h->frm.base);
        if (h->io.base) hipFree(h->io.base);
        if (h->rs.table) hipFree(h->rs.table);
        if (h->warp_G) hipFree(h->warp_G);
        if (h->warp_pin) hipHostFree(h->warp_pin);
        row_rates_drop(h);
        if (h->pin.base) hipHostFree(h->pin.base);
        if (h->d_range) hipFree(h->d_range);
        if (h->h_range) hipHostFree(h->h_range);
        for (auto &r : h->ring)
            if (r) hipHostFree(r);
        for (auto &e : h->ring_ev)
            if (e) hipEventDestroy(e);
        for (auto &p : h->conv_events) {
            hipEventDestroy(p.first);
            hipEventDestroy(p.second);
        }
        for (auto &e : h->ev)
            if (e) hipEventDestroy(e);
        if (h->stream) hipStreamDestroy(h->stream);
    }
    delete h;
}

const char *vits_last_error(vits_handle *h) { return h ? h->err.c_str() : g_open_error.c_str(); }

int vits_num_inputs(vits_handle *h) { return h ? (int)h->model.input_names.size() : 0; }
const char *vits_input_name(vits_handle *h, int i) {
    if (!h || i < 0 || i >= (int)h->model.input_names.size()) return nullptr;
    return h->model.input_names[i].c_str();
}

int vits_meta(vits_handle *h, const char *key, char *buf, size_t n) {
    if (!h || !key) return VITS_E_ARG;
    auto it = h->model.meta.find(key);
    if (it == h->model.meta.end()) return fail(h, VITS_E_ARG, "no metadata key %s", key);
    if (buf && n) {
        size_t k = it->second.size() < n - 1 ? it->second.size() : n - 1;
        std::memcpy(buf, it->second.data(), k);
        buf[k] = 0;
    }
    return (int)it->second.size();
}

int vits_hparam(vits_handle *h, const char *key, int64_t *out) {
    if (!h || !key || !out) return VITS_E_ARG;
    const Model &m = h->model;
    std::string k = key;
    if (k == "hidden") *out = m.H;
    else if (k == "inter") *out = m.C;
    else if (k == "filter") *out = m.FF;
    else if (k == "n_heads") *out = m.n_heads;
    else if (k == "n_layers") *out = m.n_layers;
    else if (k == "n_vocab") *out = m.n_vocab;
    else if (k == "n_speakers") *out = m.n_speakers;
    else if (k == "gin") *out = m.gin;
    else if (k == "gen_sx") *out = m.gen_sx ? 1 : 0;
    else if (k == "gen_nprod") *out = h->gen_nprod;
    else if (k == "enc_sx") *out = m.enc_sx ? 1 : 0;
    else if (k == "use_sdp") *out = m.use_sdp;
    else if (k == "hop") *out = m.hop;
    else if (k == "n_ups") *out = (int64_t)m.ups.size();
    else if (k == "resblock") *out = m.ups.empty() || m.ups[0].rbs.empty() ? 0 : (m.ups[0].rbs[0].type1 ? 1 : 2);
    else if (k == "window") *out = m.window;
    else if (k == "gen_rf_frames") *out = m.gen_rf_frames;
    else if (k == "upsample_initial_channel") *out = m.C0;
    else if (k == "dec_macs_per_frame") *out = (int64_t)m.dec_macs_per_frame;
    else if (k == "flow_macs_per_frame") *out = (int64_t)m.flow_macs_per_frame;
    else if (k == "enc_macs_per_token") *out = (int64_t)m.enc_macs_per_token;
    else if (k == "dec_bytes_per_frame") *out = (int64_t)(m.dec_elems_per_frame * 4);
    else if (k == "workspace_bytes") *out = (int64_t)(h->tok.cap + h->frm.cap + h->io.cap);
    else return fail(h, VITS_E_ARG, "unknown hparam %s", key);
    return VITS_OK;
}

size_t vits_arena_bytes(vits_handle *h) { return h ? (size_t)h->model.arena_floats * 4 : 0; }
const void *vits_arena_host(vits_handle *h) { return h && !h->model.arena.empty() ? h->model.arena.data() : nullptr; }
void *vits_arena_device(vits_handle *h) { return h ? h->arena_dev : nullptr; }
void *vits_stream(vits_handle *h) { return h ? (void *)h->stream : nullptr; }

int vits_set_timing(vits_handle *h, int enable) {
    if (!h) return VITS_E_ARG;
    h->timing = enable == 2 ? 2 : (enable != 0 ? 1 : 0);
    return VITS_OK;
}

int vits_set_pitch_at_rate(vits_handle *h, int on) {
    if (!h) return VITS_E_ARG;
    std::lock_guard<std::mutex> lk(h->mu);
    h->pitch_at_rate = on != 0;
    return VITS_OK;
}

int vits_set_tails(vits_handle *h, int reference) {
    if (!h) return VITS_E_ARG;
    std::lock_guard<std::mutex> lk(h->mu);
    h->tails_reference = reference != 0;
    return VITS_OK;
}

// the rate a handle's voice renders at: in_rate, or (<= 0) the file's "sample_rate" metadata, 22050 without it
static int native_rate(vits_handle *h, int in_rate) {
    if (in_rate > 0) return in_rate;
    auto it = h->model.meta.find("sample_rate");
    return it != h->model.meta.end() ? std::atoi(it->second.c_str()) : 22050;
}

// a plan's table on the handle's device, rows padded to whole 16 bytes
static int resample_table_upload(vits_handle *h, ResampleDev &d) {
    d.Kp = resample_pitch(d.plan);
    std::vector<float> t((size_t)d.plan.L * d.Kp);
    resample_table(d.plan, t.data(), d.Kp);
    if (hipSetDevice(h->device) != hipSuccess) return fail(h, VITS_E_DEVICE, "hipSetDevice(%d) failed", h->device);
    if (hipMalloc((void **)&d.table, t.size() * sizeof(float)) != hipSuccess) {
        (void)hipGetLastError();
        d.table = nullptr;
        return fail(h, VITS_E_NOMEM, "cannot place the %zu-byte resampling table on device %d", t.size() * sizeof(float), h->device);
    }
    if (hipMemcpy(d.table, t.data(), t.size() * sizeof(float), hipMemcpyHostToDevice) != hipSuccess) {
        hipFree(d.table);
        d.table = nullptr;
        return fail(h, VITS_E_DEVICE, "cannot copy the resampling table to device %d", h->device);
    }
    return 0;
}

// Drop the handle's row rates: the tables that `keep` (the setting that replaces them) did not take over, and the records.
// A run that reads them may still be in flight.
static void row_rates_drop(vits_handle *h, const vits_handle::RowRates *keep) {
    auto &old = h->rows;
    bool synced = false;
    auto sync = [&] {
        if (synced) return;
        hipSetDevice(h->device);
        hipStreamSynchronize(h->stream);
        synced = true;
    };
    for (auto &d : old.plans) {
        if (!d.table) continue;
        bool kept = false;
        for (size_t i = 0; keep && i < keep->plans.size(); i++) kept = kept || keep->plans[i].table == d.table;
        if (kept) continue;
        sync();
        hipFree(d.table);
    }
    if (old.d_recs) {
        sync();
        hipFree(old.d_recs);
    }
    old = vits_handle::RowRates{};
}

int vits_set_output_rates(vits_handle *h, int in_rate, const int32_t *out_rates, int n_rows) {
    if (!h) return VITS_E_ARG;
    std::lock_guard<std::mutex> lk(h->mu);
    if (n_rows < 0) return fail(h, VITS_E_ARG, "n_rows = %d is negative", n_rows);
    if (!out_rates || n_rows == 0) {  // clear: the row rates alone
        row_rates_drop(h);
        return VITS_OK;
    }
    vits_handle::RowRates nw;
    nw.fi = native_rate(h, in_rate);
    if (nw.fi < 1 || nw.fi > kResampleMaxRate) return fail(h, VITS_E_ARG, "sample rate %d outside [1, %d]", nw.fi, kResampleMaxRate);
    nw.fo.assign(out_rates, out_rates + n_rows);
    nw.plan_of.assign(n_rows, -1);
    // everything is validated before anything is allocated
    for (int b = 0; b < n_rows; b++) {
        const int fo = out_rates[b];
        if (fo < 0) return fail(h, VITS_E_ARG, "row %d: output rate %d is negative", b, fo);
        if (fo == 0 || fo == nw.fi) continue;  // native
        int k = 0;
        while (k < (int)nw.plans.size() && nw.plans[k].plan.fo != fo) k++;
        if (k == (int)nw.plans.size()) {
            if (k == VITS_MAX_ROW_RATES)
                return fail(h, VITS_E_ARG, "row %d: %d Hz is resampling rate number %d of this run; at most %d distinct ones are admitted "
                                           "(VITS_MAX_ROW_RATES)", b, fo, k + 1, VITS_MAX_ROW_RATES);
            ResampleDev d;
            const std::string e = resample_plan(nw.fi, fo, d.plan);
            if (!e.empty()) return fail(h, VITS_E_ARG, "row %d: %s", b, e.c_str());
            nw.plans.push_back(d);
        }
        nw.plan_of[b] = k;
    }
    if (!h->host_only) {
        // the tables: those of the setting in place are taken over, keyed by (fi, fo)
        std::vector<char> own(nw.plans.size(), 0);
        int rc = 0;
        for (size_t k = 0; k < nw.plans.size() && !rc; k++) {
            ResampleDev &d = nw.plans[k];
            for (const ResampleDev &o : h->rows.plans)
                if (o.table && o.plan.fi == d.plan.fi && o.plan.fo == d.plan.fo) {
                    d.table = o.table;
                    d.Kp = o.Kp;
                }
            if (d.table) continue;
            rc = resample_table_upload(h, d);
            own[k] = rc == 0;
        }
        std::vector<ResampleRowPlan> recs((size_t)n_rows);
        for (int b = 0; b < n_rows && !rc; b++) {
            recs[b] = resample_row_plan(nw.plan_of[b] >= 0 ? &nw.plans[nw.plan_of[b]] : nullptr);
            nw.lds = recs[b].span > nw.lds ? recs[b].span : nw.lds;
        }
        if (!rc && (hipSetDevice(h->device) != hipSuccess || hipMalloc((void **)&nw.d_recs, recs.size() * sizeof recs[0]) != hipSuccess)) {
            (void)hipGetLastError();
            nw.d_recs = nullptr;
            rc = fail(h, VITS_E_NOMEM, "cannot place %d plan records on device %d", n_rows, h->device);
        }
        if (!rc && hipMemcpy(nw.d_recs, recs.data(), recs.size() * sizeof recs[0], hipMemcpyHostToDevice) != hipSuccess)
            rc = fail(h, VITS_E_DEVICE, "cannot copy the plan records to device %d", h->device);
        if (rc) {  // refused: the previous setting stays in place
            for (size_t k = 0; k < nw.plans.size(); k++)
                if (own[k]) hipFree(nw.plans[k].table);
            if (nw.d_recs) hipFree(nw.d_recs);
            return rc;
        }
    }
    if (h->rs.table) {  // it replaces a handle rate (a run that reads the old table may still be in flight)
        hipSetDevice(h->device);
        hipStreamSynchronize(h->stream);
        hipFree(h->rs.table);
    }
    h->rs = ResampleDev{};
    row_rates_drop(h, &nw);
    h->rows = nw;
    return VITS_OK;
}

int vits_last_sample_rates(vits_handle *h, int32_t *buf, int n) {
    if (!h) return VITS_E_ARG;
    const int B = h->last_vocoder ? h->B : (int)h->h_ylen.size();
    const bool rows = (int)h->run_rates.size() == B;
    const int one = h->rs.plan.on() ? h->rs.plan.fo : native_rate(h, 0);
    for (int b = 0; b < B && b < n && buf; b++) buf[b] = rows ? h->run_rates[b] : one;
    return B;
}

int vits_set_output_rate(vits_handle *h, int in_rate, int out_rate) {
    if (!h) return VITS_E_ARG;
    std::lock_guard<std::mutex> lk(h->mu);
    if (out_rate < 0) return fail(h, VITS_E_ARG, "output rate %d is negative", out_rate);
    ResampleDev nw;  // (off)
    if (out_rate != 0) {
        const int fi = native_rate(h, in_rate);
        ResamplePlan p;
        const std::string e = resample_plan(fi, out_rate, p);
        if (!e.empty()) return fail(h, VITS_E_ARG, "%s", e.c_str());
        if (fi != out_rate) nw.plan = p;  // (equal rates: no resampling, the native path)
    }
    if (nw.plan.on() && !h->host_only) {
        nw.Kp = resample_pitch(nw.plan);
        std::vector<float> t((size_t)nw.plan.L * nw.Kp);
        resample_table(nw.plan, t.data(), nw.Kp);
        if (hipSetDevice(h->device) != hipSuccess) return fail(h, VITS_E_DEVICE, "hipSetDevice(%d) failed", h->device);
        if (hipMalloc((void **)&nw.table, t.size() * sizeof(float)) != hipSuccess) {
            (void)hipGetLastError();
            return fail(h, VITS_E_NOMEM, "cannot place the %zu-byte resampling table on device %d", t.size() * sizeof(float), h->device);
        }
        if (hipMemcpy(nw.table, t.data(), t.size() * sizeof(float), hipMemcpyHostToDevice) != hipSuccess) {
            hipFree(nw.table);
            return fail(h, VITS_E_DEVICE, "cannot copy the resampling table to device %d", h->device);
        }
    }
    if (h->rs.table) {  // (a run that reads the old table may still be in flight)
        hipSetDevice(h->device);
        hipStreamSynchronize(h->stream);
        hipFree(h->rs.table);
    }
    h->rs = nw;
    row_rates_drop(h);  // (a handle rate, or none, replaces a rate per row)
    return VITS_OK;
}

int vits_last_sample_counts(vits_handle *h, int64_t *buf, int n) {
    if (!h) return VITS_E_ARG;
    const int B = (int)h->h_ylen.size();
    const int64_t hop = h->model.hop;
    const bool rows = !h->last_vocoder && (int)h->run_L.size() == B;  // the last run had a rate per row: at ITS rates
    const bool warped = !h->last_vocoder && (int)h->warp_counts.size() == B && B > 0;  // ... was warped: its plan's counts
    for (int b = 0; b < B && b < n && buf; b++) {
        if (warped) {
            buf[b] = h->warp_counts[b];
            continue;
        }
        const int64_t s = (int64_t)h->h_ylen[b] * hop;
        buf[b] = rows ? (s * h->run_L[b] + h->run_M[b] - 1) / h->run_M[b] : h->rs.plan.on() ? h->rs.plan.count(s) : s;
    }
    return B;
}

int vits_resample_plan(int in_rate, int out_rate, int64_t *L, int64_t *M, int64_t *K, float *table, size_t table_elems) {
    ResamplePlan p;
    const std::string e = resample_plan(in_rate, out_rate, p);
    if (!e.empty()) return fail(nullptr, VITS_E_ARG, "%s", e.c_str());
    if (L) *L = p.L;
    if (M) *M = p.M;
    if (K) *K = p.K;
    if (table) {
        if (table_elems < (size_t)(p.L * p.K))
            return fail(nullptr, VITS_E_ARG, "table buffer too small: %zu < %lld", table_elems, (long long)(p.L * p.K));
        resample_table(p, table, p.K);
    }
    return VITS_OK;
}

static int check_dev(vits_handle *h) {
    if (!h) return VITS_E_ARG;
    if (h->host_only) return fail(h, VITS_E_DEVICE, "handle was opened host-only");
    if (hipSetDevice(h->device) != hipSuccess) return fail(h, VITS_E_DEVICE, "hipSetDevice(%d) failed", h->device);
    return 0;
}

int vits_reserve(vits_handle *h, int B, int T, int F) {
    if (int rc = check_dev(h)) return rc;
    std::lock_guard<std::mutex> lk(h->mu);
    const Model &m = h->model;
    if (B <= 0 || T < 0 || F < 0) return fail(h, VITS_E_ARG, "vits_reserve: B=%d T=%d F=%d", B, T, F);
    const int Fp = (F + 3) & ~3;  // (the flow runs on whole groups of 4 frames)
    if (T > 0) {
        if (int rc = slab_reserve(h, h->tok, carved_bytes([&](Carver &cv) { carve_tokens(cv, m, B, T); }), false)) return rc;
        // the staging slab: the inputs of a call, injected noises included (vits_noise) ... or, between runs,
        // vits_last_pcm16's int16 waveform and per-utterance peaks (the larger of the two uses)
        const size_t io_in = carved_bytes([&](Carver &cv) { carve_inputs(cv, m, B, T, T, Fp); });
        const size_t io_pcm = carved_bytes([&](Carver &cv) { carve_pcm16(cv, B, F * m.hop); });
        // ... or vits_deliver's, with vits_deliver_trimmed's slots, vits_deliver_leveled's buffers and vits_deliver_shaped's
        // tables behind them (two breakpoints per token: what a per-token gain needs at most)
        const int64_t shape_pts = std::min<int64_t>((int64_t)2 * B * T, kShapeMaxPoints) + B;  // (knots: a segment's points + 1)
        // ... and vits_deliver_limited's gain buffer last
        const DeliveryNeeds all{/*scan=*/true, /*levelled=*/true, /*shaped=*/true, shape_pts, /*limited=*/true};
        const size_t io_dlv = carved_bytes([&](Carver &cv) { carve_delivery_call(cv, B, F * m.hop, all); });
        // ... or a stream's (carve_stream): every chunk_frames <= F, i.e. chunks of up to the row's samples - the look-ahead the
        // last chunk delivers beyond what it renders included -, shaped for the longest look-ahead and trimmed; at an output rate K > 0
        const auto stream_bytes = [&](int64_t row, int K) {
            return carved_bytes([&](Carver &cv) { carve_stream(cv, B, row, row, K, true, true, VITS_LIMIT_MAX_LOOKAHEAD, shape_pts, /*trimmed=*/true); });
        };
        const size_t io_sp = stream_bytes((int64_t)F * m.hop, 0);
        size_t io = io_in > io_pcm ? io_in : io_pcm;
        io = io_dlv > io ? io_dlv : io;
        io = io_sp > io ? io_sp : io;
        if (h->rs.plan.on()) {  // ... or the resampled waveform with its own 16-bit rendering and delivery buffers
            const int64_t so = h->rs.plan.count((int64_t)F * m.hop);
            if (so > INT_MAX) return fail(h, VITS_E_ARG, "vits_reserve: F=%d frames are %lld samples at %d Hz", F, (long long)so, h->rs.plan.fo);
            const size_t io_rs = stream_bytes(so, (int)h->rs.plan.K);
            io = io_rs > io ? io_rs : io;
            // (a trimmed delivery's slots and a levelled one's buffers lie behind the resampled result too: in the place of
            // an encoded stream's buffers)
            const size_t io_rt = carved_bytes([&](Carver &cv) {
                const DeliveryBufs front = carve_resample(cv, B, (int)so, (int)h->rs.plan.K).dlv;
                carve_delivery_call(cv, B, (int)so, all, &front);
            });
            io = io_rt > io ? io_rt : io;
        }
        if (!h->rows.plans.empty()) {  // ... or the same at a rate per row: the longest row any plan that is set makes, the largest K
            int64_t so = (int64_t)F * m.hop;
            int K = 0;
            for (const ResampleDev &d : h->rows.plans) {
                const int64_t c = d.plan.count((int64_t)F * m.hop);
                if (c > INT_MAX) return fail(h, VITS_E_ARG, "vits_reserve: F=%d frames are %lld samples at %d Hz", F, (long long)c, d.plan.fo);
                so = c > so ? c : so;
                K = d.plan.K > K ? (int)d.plan.K : K;
            }
            const size_t io_rt = carved_bytes([&](Carver &cv) {
                const DeliveryBufs front = carve_resample(cv, B, (int)so, K).dlv;
                carve_delivery_call(cv, B, (int)so, all, &front);
            });
            io = io_rt > io ? io_rt : io;
        }
        if (int rc = slab_reserve(h, h->io, io, false)) return rc;
    }
    if (F > 0)
        if (int rc = slab_reserve(h, h->frm, carved_bytes([&](Carver &cv) { carve_frames(cv, m, B, Fp, Fp, /*flow=*/true); }), false)) return rc;
    return VITS_OK;
}

// the settings of a run: one [3] vector for the whole batch (the vits_run* entry points) ...
static RunRows one_row(const float scales[3]) {
    RunRows rr;
    rr.scales = scales;
    return rr;
}

// ... or a host [B][3] row and optionally a host [B] seed per utterance (vits_run_*_rows): every value finite, checked on
// the host before anything is enqueued; otherwise the rows accept what the [3] vector does
static int host_rows(vits_handle *h, const float *scales, int B, const uint64_t *seeds, RunRows &rr) {
    if (!scales) return fail(h, VITS_E_ARG, "null argument");
    for (int b = 0; b < B; b++) {
        const float *r = scales + (int64_t)b * 3;
        if (!std::isfinite(r[0]) || !std::isfinite(r[1]) || !std::isfinite(r[2]))
            return fail(h, VITS_E_ARG, "scales row %d = [%g, %g, %g] is not finite", b, (double)r[0], (double)r[1], (double)r[2]);
    }
    rr.scales = scales;
    rr.rows = true;
    rr.seeds = seeds;
    return VITS_OK;
}

// frames per utterance of a forced or fitted run: VITS_MAX_FORCED_FRAMES, and no more than keep its SAMPLES (frames * hop) in int
static int64_t max_forced_frames(const vits_handle *h) {
    const int64_t hop = h->model.hop > 0 ? h->model.hop : 1;
    return VITS_MAX_FORCED_FRAMES < INT_MAX / hop ? VITS_MAX_FORCED_FRAMES : INT_MAX / hop;
}

// ... with vits_controls on top: forced durations or per-token rates, host [B][T].  Everything is checked here, on the
// host, before anything is enqueued or allocated; a rejected call leaves the previous run's results readable.
static int host_controls(vits_handle *h, const vits_controls *ctl, const int64_t *lens, int B, int T, RunRows &rr) {
    if (!ctl) return fail(h, VITS_E_ARG, "null argument");
    if (B <= 0 || T <= 0) return fail(h, VITS_E_ARG, "empty batch or sequence (B=%d, T=%d)", B, T);
    if (!lens) return fail(h, VITS_E_ARG, "null argument");
    if (int rc = host_rows(h, ctl->scales_rows, B, ctl->seeds, rr)) return rc;
    if (ctl->durations && ctl->token_rate)
        return fail(h, VITS_E_ARG, "durations and token_rate are contradictory: forced durations leave nothing to scale");
    const int64_t max_frames = max_forced_frames(h);
    for (int b = 0; b < B; b++) {
        if (lens[b] < 0 || lens[b] > T)
            return fail(h, VITS_E_ARG, "input_lengths[%d]=%lld outside [0,%d]", b, (long long)lens[b], T);
        const int L = (int)lens[b];
        int64_t sum = 0;
        for (int t = 0; t < L; t++) {
            if (ctl->durations) {
                const int64_t d = ctl->durations[(int64_t)b * T + t];
                if (d < 0) return fail(h, VITS_E_ARG, "durations[%d,%d]=%lld is negative", b, t, (long long)d);
                if (d > max_frames || (sum += d) > max_frames)
                    return fail(h, VITS_E_ARG,
                                "durations[%d,%d]=%lld: utterance %d would exceed the %lld frames a forced run admits "
                                "(VITS_MAX_FORCED_FRAMES, INT_MAX / hop) at this token", b, t, (long long)d, b,
                                (long long)max_frames);
            } else if (ctl->token_rate) {
                const float r = ctl->token_rate[(int64_t)b * T + t];
                if (!std::isfinite(r) || r < 0.f)
                    return fail(h, VITS_E_ARG, "token_rate[%d,%d]=%g is not a finite value >= 0", b, t, (double)r);
            }
        }
    }
    rr.durations = ctl->durations;
    rr.token_rate = ctl->token_rate;
    return VITS_OK;
}

// ... and a vits_fit on top of the controls (vitsmi.h, "fitted durations"): pure host code, answered before the device is
// looked at.  No row in any group: rr.fit stays NULL, and the run is the entry without a fit.
static int host_fit(vits_handle *h, const vits_controls *ctl, const vits_fit *fit, int B, RunRows &rr) {
    if (!fit) return VITS_OK;
    if (B <= 0) return fail(h, VITS_E_ARG, "empty batch (B=%d)", B);
    const std::string e = fit_fault(fit, B, max_forced_frames(h));
    if (!e.empty()) return fail(h, VITS_E_ARG, "%s", e.c_str());
    if (!fit_on(fit, B)) return VITS_OK;
    if (ctl && ctl->durations)
        return fail(h, VITS_E_ARG, "durations and a fit are contradictory: forced durations leave nothing to fit");
    rr.fit = fit;
    return VITS_OK;
}

static int run_device_locked(vits_handle *h, const int64_t *ids, const int64_t *lens, int B, int T,
                             RunRows rr, const int64_t *sid, const vits_noise *noise, vits_output *out,
                             const ChunkSink *sink = nullptr) {
    if (B <= 0 || T <= 0) return fail(h, VITS_E_ARG, "empty batch or sequence (B=%d, T=%d)", B, T);
    if (!ids || !lens || !rr.scales || (!out && !sink)) return fail(h, VITS_E_ARG, "null argument");
    if (h->model.gin && !sid) return fail(h, VITS_E_ARG, "Missing speaker id");
    std::memset(&h->stats, 0, sizeof h->stats);
    h->conv_events_used = 0;
    g_launch_name_on = h->timing == 1;
    h->B = B;
    h->T = T;
    h->range_failed = false;
    h->out_resampled = false;
    forget_row_run(h);
    h->last_vocoder = false;
    uint64_t seed = noise ? noise->seed : 0;
    seed = seed * 0x9E3779B97F4A7C15ull + (++h->run_counter);
    // (run_tokens' one synchronisation also completes the previous run on this handle: its range verdict, if nobody
    // asked for it yet, is looked at there, before this run's guard slots are cleared)
    if (int rc = run_tokens(h, ids, lens, B, T, rr, sid, noise ? noise->noise_dp : nullptr, seed)) return rc;
    range_begin(h);
    if (int rc = run_frames(h, B, T, rr, sid, noise ? noise->noise_z : nullptr, noise ? noise->noise_z_stride : 0,
                            seed, sink))
        return rc;
    // a pitched run at an output rate: no resampler stage - the rate is folded into the warp's one launch
    const bool folded = rr.semitones && !sink && (h->rs.plan.on() || h->rows.on());
    if (h->rs.plan.on() && !sink && !folded)
        if (int rc = resample_run(h, h->d_ylen, B)) return rc;
    if (h->rows.on() && !sink && !folded)
        if (int rc = resample_rows_run(h, h->d_ylen, B)) return rc;
    if (rr.semitones && !sink)
        if (int rc = folded ? warp_rate_run(h, rr, B, T) : warp_run(h, rr, B, T)) return rc;
    ylen_to_i64<<<(B + 63) / 64, 64, 0, h->stream>>>(h->d_ylen, h->d_ylen64, B);
    range_end(h);
    if (out) {
        out->data = h->d_out;
        out->dims[0] = B;
        out->dims[1] = 1;
        out->dims[2] = 1;
        out->dims[3] = h->S;
        out->y_lengths = h->d_ylen64;
    }
    return VITS_OK;
}

int vits_run_device(vits_handle *h, const int64_t *ids, const int64_t *lens, int B, int T, const float scales[3],
                    const int64_t *sid, const vits_noise *noise, vits_output *out) {
    if (int rc = check_dev(h)) return rc;
    std::lock_guard<std::mutex> lk(h->mu);
    if (!out) return fail(h, VITS_E_ARG, "null argument");
    if (h->rs.plan.on()) return fail(h, VITS_E_ARG, "vits_run_device is not covered with an output rate set");
    if (int rc = row_rates_admit(h, B, "vits_run_device")) return rc;
    return run_device_locked(h, ids, lens, B, T, one_row(scales), sid, noise, out);
}

int vits_run_device_rows(vits_handle *h, const int64_t *ids, const int64_t *lens, int B, int T, const float *scales,
                         const int64_t *sid, const vits_noise *noise, const uint64_t *seeds, vits_output *out) {
    if (int rc = check_dev(h)) return rc;
    std::lock_guard<std::mutex> lk(h->mu);
    if (!out) return fail(h, VITS_E_ARG, "null argument");
    if (h->rs.plan.on()) return fail(h, VITS_E_ARG, "vits_run_device_rows is not covered with an output rate set");
    if (int rc = row_rates_admit(h, B, "vits_run_device_rows")) return rc;
    RunRows rr;
    if (int rc = host_rows(h, scales, B, seeds, rr)) return rc;
    return run_device_locked(h, ids, lens, B, T, rr, sid, noise, out);
}

int vits_last_y_lengths(vits_handle *h, int64_t *buf, int n) {
    if (!h) return VITS_E_ARG;
    int B = (int)h->h_ylen.size();
    for (int b = 0; b < B && b < n && buf; b++) buf[b] = h->h_ylen[b];
    return B;
}

int vits_last_durations(vits_handle *h, int64_t *buf, size_t n_elems) {
    if (!h) return VITS_E_ARG;
    const size_t n = (size_t)h->h_dur_B * h->h_dur_T;
    if (n == 0 || h->h_dur.size() < n) return fail(h, VITS_E_ARG, "no completed run to report durations of");
    for (size_t i = 0; i < n && i < n_elems && buf; i++) buf[i] = (int64_t)h->h_dur[i];
    return (int)n;
}

int vits_last_fit(vits_handle *h, double *scale, int64_t *frames, int32_t *status, int n) {
    if (!h) return VITS_E_ARG;
    const int G = (int)h->h_fit.size();
    if (G == 0 || h->h_dur_B == 0) return fail(h, VITS_E_ARG, "the last run was not fitted: no fit to report");
    for (int g = 0; g < G && g < n; g++) {
        if (scale) scale[g] = h->h_fit[g].scale;
        if (frames) frames[g] = h->h_fit[g].frames;
        if (status) status[g] = h->h_fit[g].status;
    }
    return G;
}

int vits_fit_plan(const float *w, const int64_t *lens, int B, int T, const vits_fit *fit, int64_t *durations, double *scale,
                  int64_t *frames, int32_t *status) {
    if (!w || !lens || !fit || !durations || B <= 0 || T <= 0) return fail(nullptr, VITS_E_ARG, "bad fit plan arguments (B=%d, T=%d) or a null pointer", B, T);
    for (int b = 0; b < B; b++)
        if (lens[b] < 0 || lens[b] > T) return fail(nullptr, VITS_E_ARG, "input_lengths[%d]=%lld outside [0,%d]", b, (long long)lens[b], T);
    const std::string e = fit_fault(fit, B, VITS_MAX_FORCED_FRAMES);
    if (!e.empty()) return fail(nullptr, VITS_E_ARG, "%s", e.c_str());
    for (int g = 0; g < fit->n_groups; g++) {
        double s;
        int64_t f;
        int32_t st;
        fit_plan_group(w, lens, fit->group, B, T, g, fit->target_frames[g], fit->mode[g], durations, s, f, st);
        if (scale) scale[g] = s;
        if (frames) frames[g] = f;
        if (status) status[g] = st;
    }
    return VITS_OK;
}

int vits_sync(vits_handle *h) {
    if (int rc = check_dev(h)) return rc;
    std::lock_guard<std::mutex> lk(h->mu);
    HIPCHECK(h, hipStreamSynchronize(h->stream));
    if (int rc = range_check(h)) return rc;
    if (h->range_failed) return fail(h, VITS_E_RANGE, "the last run left the range of the fp16 operand planes (see vits_get_stats)");
    return VITS_OK;
}

// vits_run / vits_run_chunked: validate the host inputs and stage them on the device (one slab, reused across calls)
struct Staged {
    int64_t *d_ids = nullptr, *d_lens = nullptr, *d_sid = nullptr;
    vits_noise dn{};
    bool has_noise = false;
};

static int stage_inputs(vits_handle *h, const int64_t *ids, const int64_t *lens, int B, int T, const int64_t *sid,
                        const vits_noise *noise, Staged &sg) {
    if (B <= 0 || T <= 0) return fail(h, VITS_E_ARG, "empty batch or sequence (B=%d, T=%d)", B, T);
    if (!ids || !lens) return fail(h, VITS_E_ARG, "null argument");
    const Model &m = h->model;
    for (int b = 0; b < B; b++) {
        if (lens[b] < 0 || lens[b] > T)
            return fail(h, VITS_E_ARG, "input_lengths[%d]=%lld outside [0,%d]", b, (long long)lens[b], T);
        for (int t = 0; t < T; t++) {
            int64_t id = ids[(int64_t)b * T + t];
            if (id < 0 || id >= m.n_vocab)
                return fail(h, VITS_E_ARG, "phoneme id %lld at [%d,%d] is out of range [0,%d)", (long long)id, b, t,
                            m.n_vocab);
        }
        if (sid && m.gin && (sid[b] < 0 || sid[b] >= m.n_speakers))
            return fail(h, VITS_E_ARG, "sid[%d]=%lld is out of range [0,%d)", b, (long long)sid[b], m.n_speakers);
    }
    if (m.gin && !sid) return fail(h, VITS_E_ARG, "Missing speaker id");
    const int64_t Fz = noise && noise->noise_z ? noise->noise_z_stride : 0;
    const int Tdp = noise && noise->noise_dp ? T : 0;
    const size_t ndp = (size_t)B * 2 * Tdp * 4, nz = (size_t)B * m.C * Fz * 4;
    InputBufs in;
    if (int rc0 = slab_carve(h, h->io, "staging", [&](Carver &cv) { in = carve_inputs(cv, m, B, T, Tdp, Fz); })) return rc0;
    if (h->out_resampled) forget_results_in(h, h->io);  // (a resampled waveform lived where these inputs go)
    sg.d_ids = in.ids;
    sg.d_lens = in.lens;
    int64_t *d_sid = in.sid;
    float *d_ndp = in.noise_dp, *d_nz = in.noise_z;
    hipStream_t st = h->stream;
    int rc = VITS_OK;
    auto cp = [&](void *d, const void *s, size_t n) {
        if (rc == VITS_OK && hipMemcpyAsync(d, s, n, hipMemcpyHostToDevice, st) != hipSuccess)
            rc = fail(h, VITS_E_DEVICE, "host-to-device copy failed");
    };
    {
        // ids | lens | sid are contiguous on the device: gather them in pinned memory and send them as one copy
        const size_t n_ids = (size_t)B * T * 8, n_b = (size_t)B * 8, n_all = n_ids + n_b + (sid ? n_b : 0);
        if (h->h_in_pin_bytes < n_all) {
            if (h->h_in_pin) hipHostFree(h->h_in_pin);
            h->h_in_pin = nullptr;
            h->h_in_pin_bytes = 0;
            const size_t cap = n_all < 65536 ? 65536 : n_all;
            if (hipHostMalloc((void **)&h->h_in_pin, cap) == hipSuccess) h->h_in_pin_bytes = cap;
        }
        if (h->h_in_pin_bytes >= n_all) {
            // (the previous call's copy out of this buffer has completed: every call ends its input phase with a stream sync)
            std::memcpy(h->h_in_pin, ids, n_ids);
            std::memcpy(h->h_in_pin + n_ids, lens, n_b);
            if (sid) std::memcpy(h->h_in_pin + n_ids + n_b, sid, n_b);
            cp(sg.d_ids, h->h_in_pin, n_all);
        } else {
            cp(sg.d_ids, ids, n_ids);
            cp(sg.d_lens, lens, n_b);
            if (sid) cp(d_sid, sid, n_b);
        }
        if (sid) sg.d_sid = d_sid;
    }
    if (noise) {
        sg.has_noise = true;
        sg.dn = *noise;
        if (noise->noise_dp) {
            cp(d_ndp, noise->noise_dp, ndp);
            sg.dn.noise_dp = d_ndp;
        }
        if (noise->noise_z) {
            cp(d_nz, noise->noise_z, nz);
            sg.dn.noise_z = d_nz;
        }
    }
    return rc;
}

// host inputs in; returns once everything is enqueued (the mid-pipeline frame-count readback has completed, and with it
// the input copies: the caller's buffers are free)
static int run_async_locked(vits_handle *h, const int64_t *ids, const int64_t *lens, int B, int T, const RunRows &rr,
                            const int64_t *sid, const vits_noise *noise, vits_output *dev) {
    if (!rr.scales) return fail(h, VITS_E_ARG, "null argument");
    if (int rc = row_rates_admit(h, B, nullptr)) return rc;
    Staged sg;
    int rc = stage_inputs(h, ids, lens, B, T, sid, noise, sg);
    if (rc == VITS_OK) rc = run_device_locked(h, sg.d_ids, sg.d_lens, B, T, rr, sg.d_sid, sg.has_noise ? &sg.dn : nullptr, dev);
    if (rc != VITS_OK) hipStreamSynchronize(h->stream);  // the staging slab is reused by the next call
    return rc;
}

static int run_chunked_sink(vits_handle *h, const int64_t *ids, const int64_t *lens, int B, int T, const RunRows &rr,
                            const int64_t *sid, const vits_noise *noise, const ChunkSink &sink) {
    if (!rr.scales || sink.chunk_frames < 1) return fail(h, VITS_E_ARG, "bad chunked-run arguments");
    if (int rc = row_rates_admit(h, B, "a chunked run")) return rc;
    Staged sg;
    int rc = stage_inputs(h, ids, lens, B, T, sid, noise, sg);
    if (rc == VITS_OK)
        rc = run_device_locked(h, sg.d_ids, sg.d_lens, B, T, rr, sg.d_sid, sg.has_noise ? &sg.dn : nullptr, nullptr, &sink);
    if (hipStreamSynchronize(h->stream) != hipSuccess && rc == VITS_OK)
        rc = fail(h, VITS_E_DEVICE, "synchronisation failed: %s", hipGetErrorString(hipGetLastError()));
    // (chunks are handed out as they finish; a range violation is therefore reported after the fact)
    if (rc == VITS_OK) rc = range_check(h);
    return rc;
}

// vits_stream_format, checked on the host before anything else looks at the call (vitsmi.h, "encoded streaming")
static int host_stream_format(vits_handle *h, const vits_stream_format *fmt, int B) {
    if (!fmt) return fail(h, VITS_E_ARG, "null stream format");
    if (fmt->encoding < VITS_ENC_PCM16 || fmt->encoding > VITS_ENC_F32) return fail(h, VITS_E_ARG, "unknown encoding %d", (int)fmt->encoding);
    for (int b = 0; b < B; b++) {
        if (fmt->volume && !std::isfinite(fmt->volume[b])) return fail(h, VITS_E_ARG, "volume[%d] = %g is not finite", b, (double)fmt->volume[b]);
        if (fmt->ref_peak && !(std::isfinite(fmt->ref_peak[b]) && fmt->ref_peak[b] >= 0.f))
            return fail(h, VITS_E_ARG, "ref_peak[%d] = %g is not a finite value >= 0", b, (double)fmt->ref_peak[b]);
    }
    return VITS_OK;
}

// vits_stream_shaping, checked on the host behind the format (vitsmi.h, "shaped streaming")
static int host_stream_shaping(vits_handle *h, const vits_stream_shaping *shaping, const vits_stream_format *fmt, int B) {
    const std::string e = stream_shape_fault(shaping, fmt ? fmt->volume : nullptr, B);
    if (!e.empty()) return fail(h, VITS_E_ARG, "%s", e.c_str());
    return VITS_OK;
}

int vits_stream_shaping_check(const vits_stream_shaping *shaping, const vits_stream_format *fmt, int B) {
    if (B < 0) return fail(nullptr, VITS_E_ARG, "B = %d is negative", B);
    return host_stream_shaping(nullptr, shaping, fmt, B);
}

int vits_stream_emit_range(int64_t first, int64_t n, int is_last, int64_t total, int lookahead, int64_t *e_first, int64_t *e_n) {
    if (!e_first || !e_n || first < 0 || n < 0 || total < 0 || first + n > total || lookahead < 0 || lookahead > VITS_LIMIT_MAX_LOOKAHEAD)
        return fail(nullptr, VITS_E_ARG, "bad emit range arguments: piece [%lld, +%lld) of %lld, lookahead %d", (long long)first, (long long)n,
                    (long long)total, lookahead);
    stream_emit_range(first, n, is_last != 0, total, lookahead, *e_first, *e_n);
    return VITS_OK;
}

// vits_stream_onset, checked on the host behind the shaping (vitsmi.h, "trimmed streaming")
static int host_stream_onsets(vits_handle *h, const vits_stream_onset *onsets, const vits_stream_format *fmt, int B) {
    const std::string e = stream_onset_fault(onsets, fmt ? fmt->ref_peak : nullptr, B);
    if (!e.empty()) return fail(h, VITS_E_ARG, "%s", e.c_str());
    return VITS_OK;
}

int vits_stream_onset_check(const vits_stream_onset *onsets, const vits_stream_format *fmt, int B) {
    if (B < 0) return fail(nullptr, VITS_E_ARG, "B = %d is negative", B);
    return host_stream_onsets(nullptr, onsets, fmt, B);
}

int vits_stream_onset_start(int64_t f, int64_t keep_lead, int64_t delivered_before, int64_t *a) {
    if (!a || f < 0 || keep_lead < 0 || delivered_before < 0 || delivered_before > f)
        return fail(nullptr, VITS_E_ARG, "bad onset start arguments: f %lld, keep_lead %lld, delivered_before %lld", (long long)f,
                    (long long)keep_lead, (long long)delivered_before);
    *a = stream_onset_start(f, keep_lead, delivered_before);
    return VITS_OK;
}

// the sink of an encoded entry, whole path or vocoder: its chunks go to the entry's one callback - `fn`, or `tfn` with the rows' skips
static ChunkSink encoded_sink(int chunk_frames, const vits_stream_format *fmt, const vits_stream_shaping *shaping,
                              const vits_stream_onset *onsets, vits_enc_chunk_fn fn, vits_enc_chunk_trim_fn tfn, void *user) {
    return ChunkSink{chunk_frames, nullptr, user, fmt, fn, shaping, onsets, tfn};
}

// ... and its stream arguments, checked in their one order (pure host code: a host-only handle answers it too)
static int host_stream(vits_handle *h, const ChunkSink &sink, int B) {
    if (int rc = host_stream_format(h, sink.fmt, B)) return rc;
    if (int rc = host_stream_shaping(h, sink.shaping, sink.fmt, B)) return rc;
    return host_stream_onsets(h, sink.onsets, sink.fmt, B);
}

// vits_run_async_ctl with the intonation on top (vitsmi.h, "intonation").  What is pure host code - the semitones, the
// contradictions, the rates that are set - is answered before the device is looked at: a host-only handle answers it too.
// One body serves every entry with pitch: st0 the start values (NULL: zeros), st1 the end values (NULL: every token keeps its
// speed - the warp's entry); `entry` names the caller in the refusal of an output rate.
// what host_intonation makes of a call: the controls with compensate's duration multiplier folded in, and the values a warped run plans from
struct Intoned {
    vits_controls ctl{};
    std::vector<float> rate, zeros;
    const float *st0 = nullptr, *st1 = nullptr;  // st1 == nullptr: equal ends everywhere - the warp itself
    bool warped = false;
    void apply(RunRows &rr, const int64_t *lens) const {
        if (!warped) return;
        rr.semitones = st0;
        rr.semitones_end = st1;
        rr.semitone_lens = lens;
    }
};

static int host_intonation(vits_handle *h, const vits_controls *ctl, const int64_t *lens, int B, int T, const float *st0, const float *st1,
                           int compensate, const char *entry, bool chunked, Intoned &in) {
    if (!ctl) return fail(h, VITS_E_ARG, "null argument");
    bool warped = false, glided = false;
    if (st0 || st1) {
        if (B <= 0 || T <= 0) return fail(h, VITS_E_ARG, "empty batch or sequence (B=%d, T=%d)", B, T);
        if (!lens) return fail(h, VITS_E_ARG, "null argument");
        for (int b = 0; b < B; b++) {
            if (lens[b] < 0 || lens[b] > T) return fail(h, VITS_E_ARG, "input_lengths[%d]=%lld outside [0,%d]", b, (long long)lens[b], T);
            for (int t = 0; t < (int)lens[b]; t++) {
                const float v = st0 ? st0[(int64_t)b * T + t] : 0.f, w = st1 ? st1[(int64_t)b * T + t] : v;
                int64_t step, c;
                int32_t Kh;
                if (!warp_token(v, step, c, Kh))
                    return fail(h, VITS_E_ARG, "token_semitones[%d,%d]=%g is not a finite value within [-12, 12]", b, t, (double)v);
                if (!warp_token(w, step, c, Kh))
                    return fail(h, VITS_E_ARG, "token_semitones_end[%d,%d]=%g is not a finite value within [-12, 12]", b, t, (double)w);
                warped = warped || v != 0.f || w != 0.f;
                glided = glided || v != w;
            }
        }
    }
    in.ctl = *ctl;
    in.warped = warped;
    if (!warped) return VITS_OK;
    if (compensate && ctl->durations)
        return fail(h, VITS_E_ARG, "compensate and forced durations are contradictory: forced durations are the rendered ones");
    // An output rate is refused unless the handle asked for it to be folded into the steps (vits_set_pitch_at_rate; "pitch at an
    // output rate"): then a whole run takes it where every PITCHED row's ratio lies within [1/4, 4]; a chunked run takes one rate
    // for all rows, not a rate per row.
    if ((h->rs.plan.on() || h->rows.on()) && !h->pitch_at_rate) return fail(h, VITS_E_ARG, "%s is not covered with an output rate set", entry);
    if (chunked && h->rows.on()) return fail(h, VITS_E_ARG, "%s is not covered with an output rate set per row", entry);
    for (int b = 0; b < B && (h->rs.plan.on() || h->rows.on()); b++) {
        const ResampleDev *d = rate_of_row(h, b);
        if (!d || warp_rate_ok(d->plan.L, d->plan.M)) continue;
        const float *r0 = st0 ? st0 + (int64_t)b * T : nullptr, *r1 = st1 ? st1 + (int64_t)b * T : nullptr;
        if (!warp_rate_unpitched(r0, r1 ? r1 : r0, (int)lens[b]))
            return fail(h, VITS_E_ARG, "row %d: pitch at %d -> %d Hz is not covered: the ratio of the rates lies outside [1/4, 4]", b, d->plan.fi,
                        d->plan.fo);
    }
    if (!st0) {
        in.zeros.assign((size_t)B * T, 0.f);
        st0 = in.zeros.data();
    }
    if (compensate) {  // the duration multiplier of token t: token_rate * (float)r_t - r_t the mean of its ends -, one fp32 product
        in.rate.assign((size_t)B * T, 1.0f);
        for (int b = 0; b < B; b++)
            for (int t = 0; t < (int)lens[b]; t++) {
                const size_t i = (size_t)b * T + t;
                const double r0 = std::exp2((double)st0[i] / 12.0);
                const float r = glided ? (float)((r0 + std::exp2((double)st1[i] / 12.0)) * 0.5) : (float)r0;
                in.rate[i] = (ctl->token_rate ? ctl->token_rate[i] : 1.0f) * r;
            }
        in.ctl.token_rate = in.rate.data();
    }
    in.st0 = st0;
    in.st1 = glided ? st1 : nullptr;  // equal ends: the warp itself
    return VITS_OK;
}

// One request of the whole path: what a vits_run / vits_run_async* / vits_run_chunked* entry may pass, and where its audio goes.
// Every such entry fills one - the head by position, the rest through the setters - and hands it to run_call.
struct RunCall {
    const int64_t *ids, *lens;
    int B, T;
    const int64_t *sid;
    const vits_noise *noise;
    // the settings: one [3] vector for the whole batch, or [B][3] rows and seeds, or a vits_controls
    enum { kScales, kRows, kControls } settings = kScales;
    const float *scales = nullptr;
    const uint64_t *seeds = nullptr;
    const vits_controls *ctl = nullptr;
    const vits_fit *fit = nullptr;  // on top of the controls, nullable (vitsmi.h, "fitted durations")
    // ... or the intonation on top of them: `entry` names an entry that takes one, st0 / st1 as host_intonation
    const char *entry = nullptr;
    const float *st0 = nullptr, *st1 = nullptr;
    int compensate = 0;
    // where the audio goes: it stays on the device (`dev`, if set, learns where), or fp32 chunks, or encoded ones (encoded_sink)
    enum { kAsync, kChunks, kEncoded } out = kAsync;
    vits_output *dev = nullptr;
    ChunkSink sink{};

    RunCall &one_row(const float *s) { scales = s; return *this; }
    RunCall &rows(const float *s, const uint64_t *sd) { settings = kRows; scales = s; seeds = sd; return *this; }
    RunCall &controls(const vits_controls *c, const vits_fit *f = nullptr) { settings = kControls; ctl = c; fit = f; return *this; }
    RunCall &contour(const char *name, const float *a, const float *b, int comp) { entry = name; st0 = a; st1 = b; compensate = comp; return *this; }
    RunCall &glided(const char *name, const vits_contour *c) {
        return c ? contour(name, c->token_semitones, c->token_semitones_end, c->compensate) : contour(name, nullptr, nullptr, 0);
    }
    RunCall &chunks(int chunk_frames, vits_chunk_fn fn, void *user) { out = kChunks; sink = ChunkSink{chunk_frames, fn, user}; return *this; }
    RunCall &encoded(const ChunkSink &s) { out = kEncoded; sink = s; return *this; }
};

// The one order in which a call's faults are reported; a step is taken by the entries that have its argument.  What is pure
// host code about the stream, the fit and the intonation is answered before the device is looked at - a host-only handle
// answers it too -; the settings themselves (host_controls / host_rows) are looked at behind the device.
static int run_call_locked(vits_handle *h, const RunCall &c) {
    if (c.out == RunCall::kEncoded)
        if (int rc = host_stream(h, c.sink, c.B)) return rc;
    RunRows rr;
    if (int rc = host_fit(h, c.ctl, c.fit, c.B, rr)) return rc;
    Intoned in;
    if (c.entry)
        if (int rc = host_intonation(h, c.ctl, c.lens, c.B, c.T, c.st0, c.st1, c.compensate, c.entry, c.out != RunCall::kAsync, in)) return rc;
    if (int rc = check_dev(h)) return rc;
    if (c.settings == RunCall::kScales) rr = one_row(c.scales);
    else if (c.settings == RunCall::kRows) {
        if (int rc = host_rows(h, c.scales, c.B, c.seeds, rr)) return rc;
    } else if (int rc = host_controls(h, c.entry ? &in.ctl : c.ctl, c.lens, c.B, c.T, rr)) return rc;
    in.apply(rr, c.lens);
    if (c.out != RunCall::kAsync) return run_chunked_sink(h, c.ids, c.lens, c.B, c.T, rr, c.sid, c.noise, c.sink);
    vits_output dev{};
    return run_async_locked(h, c.ids, c.lens, c.B, c.T, rr, c.sid, c.noise, c.dev ? c.dev : &dev);
}

static int run_call(vits_handle *h, const RunCall &c) {
    if (!h) return VITS_E_ARG;
    std::lock_guard<std::mutex> lk(h->mu);
    return run_call_locked(h, c);
}

int vits_run_async(vits_handle *h, const int64_t *ids, const int64_t *lens, int B, int T, const float scales[3],
                   const int64_t *sid, const vits_noise *noise) {
    return run_call(h, RunCall{ids, lens, B, T, sid, noise}.one_row(scales));
}

int vits_run_async_rows(vits_handle *h, const int64_t *ids, const int64_t *lens, int B, int T, const float *scales,
                        const int64_t *sid, const vits_noise *noise, const uint64_t *seeds) {
    return run_call(h, RunCall{ids, lens, B, T, sid, noise}.rows(scales, seeds));
}

int vits_run_async_ctl(vits_handle *h, const int64_t *ids, const int64_t *lens, int B, int T, const int64_t *sid,
                       const vits_noise *noise, const vits_controls *ctl) {
    return run_call(h, RunCall{ids, lens, B, T, sid, noise}.controls(ctl));
}

// vits_run_async_ctl / vits_run_chunked_ctl with a fit on top (vitsmi.h, "fitted durations")
int vits_run_async_fitted(vits_handle *h, const int64_t *ids, const int64_t *lens, int B, int T, const int64_t *sid,
                          const vits_noise *noise, const vits_controls *ctl, const vits_fit *fit) {
    return run_call(h, RunCall{ids, lens, B, T, sid, noise}.controls(ctl, fit));
}

int vits_run_async_warped(vits_handle *h, const int64_t *ids, const int64_t *lens, int B, int T, const int64_t *sid,
                          const vits_noise *noise, const vits_controls *ctl, const vits_intonation *into) {
    return run_call(h, RunCall{ids, lens, B, T, sid, noise}.controls(ctl).contour(
                           "vits_run_async_warped", into ? into->token_semitones : nullptr, nullptr, into ? into->compensate : 0));
}

// ... and with a start and an end value per token (vitsmi.h, "pitch contours"): equal ends everywhere are the call above
int vits_run_async_glided(vits_handle *h, const int64_t *ids, const int64_t *lens, int B, int T, const int64_t *sid,
                          const vits_noise *noise, const vits_controls *ctl, const vits_contour *contour) {
    return run_call(h, RunCall{ids, lens, B, T, sid, noise}.controls(ctl).glided("vits_run_async_glided", contour));
}

int vits_run(vits_handle *h, const int64_t *ids, const int64_t *lens, int B, int T, const float scales[3],
             const int64_t *sid, const vits_noise *noise, vits_output *out) {
    if (!h) return VITS_E_ARG;
    std::lock_guard<std::mutex> lk(h->mu);
    vits_output dev{};
    RunCall c = RunCall{ids, lens, B, T, sid, noise}.one_row(scales);
    c.dev = &dev;
    int rc = run_call_locked(h, c);  // (out == NULL: run only)
    hipStream_t st = h->stream;
    if (rc == VITS_OK && !out) {
        // run only: the caller fetches what it needs afterwards (vits_last_pcm16, vits_last_y_lengths, vits_tap)
        if (hipStreamSynchronize(st) != hipSuccess)
            rc = fail(h, VITS_E_DEVICE, "synchronisation failed: %s", hipGetErrorString(hipGetLastError()));
        else
            rc = range_check(h);
    } else if (rc == VITS_OK) {
        // one pinned block: [samples | frame counts]
        const size_t n = (size_t)B * h->S, ybase = (n * 4 + 63) & ~size_t(63);
        char *host = (char *)pinned_get(h, ybase + (size_t)B * 8);
        if (!host)
            rc = fail(h, VITS_E_NOMEM, "cannot allocate pinned output (%zu bytes)", n * 4);
        else if (hipMemcpyAsync(host, dev.data, n * 4, hipMemcpyDeviceToHost, st) != hipSuccess ||
                 hipStreamSynchronize(st) != hipSuccess) {
            pinned_put(h, host);
            rc = fail(h, VITS_E_DEVICE, "device-to-host copy failed: %s", hipGetErrorString(hipGetLastError()));
        } else if ((rc = range_check(h)) != VITS_OK) {
            pinned_put(h, host);  // clamped audio is not handed out
        } else {
            int64_t *hy = (int64_t *)(host + ybase);
            for (int b = 0; b < B; b++) hy[b] = h->h_ylen[b];
            out->data = (float *)host;
            std::memcpy(out->dims, dev.dims, sizeof dev.dims);
            out->y_lengths = hy;
        }
        if (rc != VITS_OK) hipStreamSynchronize(st);
    }
    return rc;
}

int vits_run_chunked(vits_handle *h, const int64_t *ids, const int64_t *lens, int B, int T, const float scales[3],
                     const int64_t *sid, const vits_noise *noise, int chunk_frames, vits_chunk_fn fn, void *user) {
    return run_call(h, RunCall{ids, lens, B, T, sid, noise}.one_row(scales).chunks(chunk_frames, fn, user));
}

int vits_run_chunked_rows(vits_handle *h, const int64_t *ids, const int64_t *lens, int B, int T, const float *scales,
                          const int64_t *sid, const vits_noise *noise, const uint64_t *seeds, int chunk_frames,
                          vits_chunk_fn fn, void *user) {
    return run_call(h, RunCall{ids, lens, B, T, sid, noise}.rows(scales, seeds).chunks(chunk_frames, fn, user));
}

int vits_run_chunked_ctl(vits_handle *h, const int64_t *ids, const int64_t *lens, int B, int T, const int64_t *sid,
                         const vits_noise *noise, const vits_controls *ctl, int chunk_frames, vits_chunk_fn fn, void *user) {
    return run_call(h, RunCall{ids, lens, B, T, sid, noise}.controls(ctl).chunks(chunk_frames, fn, user));
}

int vits_run_chunked_fitted(vits_handle *h, const int64_t *ids, const int64_t *lens, int B, int T, const int64_t *sid,
                            const vits_noise *noise, const vits_controls *ctl, const vits_fit *fit, int chunk_frames,
                            vits_chunk_fn fn, void *user) {
    return run_call(h, RunCall{ids, lens, B, T, sid, noise}.controls(ctl, fit).chunks(chunk_frames, fn, user));
}

// The chunked entries with pitch (vitsmi.h, "streamed pitch"): the checks are the whole run's (host_intonation), before anything is
// enqueued.  All-zero semitones leave rr without them: the call then is vits_run_chunked_ctl / vits_run_chunked_enc* itself.
int vits_run_chunked_glided(vits_handle *h, const int64_t *ids, const int64_t *lens, int B, int T, const int64_t *sid, const vits_noise *noise,
                            const vits_controls *ctl, const vits_contour *contour, int chunk_frames, vits_chunk_fn fn, void *user) {
    return run_call(h, RunCall{ids, lens, B, T, sid, noise}.controls(ctl).glided("vits_run_chunked_glided", contour).chunks(chunk_frames, fn, user));
}

// The encoded entries of the whole path: the plain callback without onsets, the trimmed one with the rows' skips
int vits_run_chunked_enc_shaped(vits_handle *h, const int64_t *ids, const int64_t *lens, int B, int T, const int64_t *sid,
                                const vits_noise *noise, const vits_controls *ctl, const vits_stream_format *fmt,
                                const vits_stream_shaping *shaping, int chunk_frames, vits_enc_chunk_fn fn, void *user) {
    return run_call(h, RunCall{ids, lens, B, T, sid, noise}.controls(ctl).encoded(
                           encoded_sink(chunk_frames, fmt, shaping, nullptr, fn, nullptr, user)));
}

int vits_run_chunked_enc(vits_handle *h, const int64_t *ids, const int64_t *lens, int B, int T, const int64_t *sid,
                         const vits_noise *noise, const vits_controls *ctl, const vits_stream_format *fmt, int chunk_frames,
                         vits_enc_chunk_fn fn, void *user) {
    return vits_run_chunked_enc_shaped(h, ids, lens, B, T, sid, noise, ctl, fmt, nullptr, chunk_frames, fn, user);
}

int vits_run_chunked_enc_fitted(vits_handle *h, const int64_t *ids, const int64_t *lens, int B, int T, const int64_t *sid,
                                const vits_noise *noise, const vits_controls *ctl, const vits_stream_format *fmt,
                                const vits_stream_shaping *shaping, const vits_stream_onset *onsets, const vits_fit *fit,
                                int chunk_frames, vits_enc_chunk_trim_fn fn, void *user) {
    return run_call(h, RunCall{ids, lens, B, T, sid, noise}.controls(ctl, fit).encoded(
                           encoded_sink(chunk_frames, fmt, shaping, onsets, nullptr, fn, user)));
}

int vits_run_chunked_enc_trimmed(vits_handle *h, const int64_t *ids, const int64_t *lens, int B, int T, const int64_t *sid,
                                 const vits_noise *noise, const vits_controls *ctl, const vits_stream_format *fmt,
                                 const vits_stream_shaping *shaping, const vits_stream_onset *onsets, int chunk_frames,
                                 vits_enc_chunk_trim_fn fn, void *user) {
    return vits_run_chunked_enc_fitted(h, ids, lens, B, T, sid, noise, ctl, fmt, shaping, onsets, nullptr, chunk_frames, fn, user);
}

int vits_run_chunked_enc_glided(vits_handle *h, const int64_t *ids, const int64_t *lens, int B, int T, const int64_t *sid,
                                const vits_noise *noise, const vits_controls *ctl, const vits_stream_format *fmt,
                                const vits_stream_shaping *shaping, const vits_stream_onset *onsets, const vits_contour *contour,
                                int chunk_frames, vits_enc_chunk_trim_fn fn, void *user) {
    return run_call(h, RunCall{ids, lens, B, T, sid, noise}.controls(ctl).glided("vits_run_chunked_enc_glided", contour).encoded(
                           encoded_sink(chunk_frames, fmt, shaping, onsets, nullptr, fn, user)));
}

int vits_last_token_spans(vits_handle *h, int64_t *buf, size_t n_elems) {
    if (!h) return VITS_E_ARG;
    const size_t n = h->warp_spans.size();
    if (n == 0 || h->warp_counts.empty()) return fail(h, VITS_E_ARG, "the last run was not warped: no token spans to report");
    for (size_t i = 0; i < n && i < n_elems && buf; i++) buf[i] = h->warp_spans[i];
    return (int)n;
}

int vits_warp_token(float semitones, int64_t *step, int64_t *cutoff, int32_t *half_taps) {
    int64_t s, c;
    int32_t Kh;
    if (!warp_token(semitones, s, c, Kh)) return fail(nullptr, VITS_E_ARG, "semitones %g is not a finite value within [-12, 12]", (double)semitones);
    if (step) *step = s;
    if (cutoff) *cutoff = c;
    if (half_taps) *half_taps = Kh;
    return VITS_OK;
}

int vits_warp_plan(const int64_t *durations, const float *semitones, int len, int hop, vits_warp_seg *segs, int64_t *spans, int64_t *n_out) {
    if (len < 0 || hop < 1 || (len > 0 && !durations)) return fail(nullptr, VITS_E_ARG, "bad warp plan arguments (len = %d, hop = %d)", len, hop);
    int64_t ns = 0, N = 0;
    const std::string e = warp_plan(durations, semitones, len, hop, segs, spans, ns, N);
    if (!e.empty()) return fail(nullptr, VITS_E_ARG, "%s", e.c_str());
    if (n_out) *n_out = N;
    return (int)ns;
}

int vits_glide_token(float st0, float st1, int64_t *step0, int64_t *step1, float *rate) {
    int64_t a, b;
    float r;
    int bad = 0;
    if (!glide_token(st0, st1, a, b, r, &bad))
        return fail(nullptr, VITS_E_ARG, "semitones %g is not a finite value within [-12, 12]", (double)(bad ? st1 : st0));
    if (step0) *step0 = a;
    if (step1) *step1 = b;
    if (rate) *rate = r;
    return VITS_OK;
}

int vits_glide_cutoff(int64_t step, int64_t *c, int32_t *half_taps) {
    if (step < kWarpMinStep || step > kWarpMaxStep)
        return fail(nullptr, VITS_E_ARG, "step %lld outside [%lld, %lld]", (long long)step, (long long)kWarpMinStep, (long long)kWarpMaxStep);
    int32_t c32, Kh;
    glide_cutoff(step, c32, Kh);
    if (c) *c = c32;
    if (half_taps) *half_taps = Kh;
    return VITS_OK;
}

int vits_glide_plan(const int64_t *durations, const float *st0, const float *st1, int len, int hop, vits_glide_seg *segs, int64_t *spans,
                    int64_t *n_out) {
    if (len < 0 || hop < 1 || (len > 0 && !durations)) return fail(nullptr, VITS_E_ARG, "bad glide plan arguments (len = %d, hop = %d)", len, hop);
    int64_t ns = 0, N = 0;
    const std::string e = glide_plan(durations, st0, st1, len, hop, segs, spans, ns, N);
    if (!e.empty()) return fail(nullptr, VITS_E_ARG, "%s", e.c_str());
    if (n_out) *n_out = N;
    return (int)ns;
}

// the emit rule of a row (vitsmi.h, "streamed pitch"), without a handle
extern "C++" {
template <class Seg, class Fault>
static int emit_end_as(const Seg *segs, int n_segs, int64_t n_in, int64_t n_out, int64_t X, int64_t *ready, Fault fault) {
    if (n_segs < 0 || (n_segs > 0 && !segs) || n_in < 0 || n_out < 0 || X < 0 || !ready)
        return fail(nullptr, VITS_E_ARG, "bad emit end arguments (n_segs = %d, n_in = %lld, n_out = %lld, X = %lld)", n_segs, (long long)n_in,
                    (long long)n_out, (long long)X);
    const std::string e = fault(segs, n_segs);
    if (!e.empty()) return fail(nullptr, VITS_E_ARG, "%s", e.c_str());
    const int64_t N = n_segs > 0 ? segs[n_segs - 1].n0 + segs[n_segs - 1].k : n_in;
    if (n_out != N) return fail(nullptr, VITS_E_ARG, "n_out = %lld, the row's records give %lld", (long long)n_out, (long long)N);
    *ready = warp_emit_row(segs, n_segs, n_in, n_out, X);
    return VITS_OK;
}
}  // extern "C++"

int vits_warp_emit_end(const vits_warp_seg *segs, int n_segs, int64_t n_in, int64_t n_out, int64_t X, int64_t *ready) {
    return emit_end_as(segs, n_segs, n_in, n_out, X, ready, warp_segs_fault);
}

int vits_glide_emit_end(const vits_glide_seg *segs, int n_segs, int64_t n_in, int64_t n_out, int64_t X, int64_t *ready) {
    return emit_end_as(segs, n_segs, n_in, n_out, X, ready, glide_segs_fault);
}

int64_t vits_warp_stream_cap(int64_t piece_samples, int64_t S_w) {
    if (piece_samples < 1 || S_w < 1) return fail(nullptr, VITS_E_ARG, "bad stream cap arguments (%lld, %lld)", (long long)piece_samples, (long long)S_w);
    return warp_stream_cap(piece_samples, S_w);
}

// ---- the folded plan (vitsmi.h, "pitch at an output rate"), without a handle

static int rate_ratio_fault(int64_t L, int64_t M) {
    if (warp_rate_ok(L, M)) return VITS_OK;
    return fail(nullptr, VITS_E_ARG, "rate ratio L / M = %lld / %lld outside [1/4, 4]", (long long)L, (long long)M);
}

int vits_warp_token_rate(float semitones, int64_t L, int64_t M, int64_t *step, int64_t *cutoff, int32_t *half_taps) {
    if (int rc = rate_ratio_fault(L, M)) return rc;
    int64_t s, c;
    int32_t Kh;
    if (!warp_token_rate(semitones, L, M, s, c, Kh))
        return fail(nullptr, VITS_E_ARG, "semitones %g is not a finite value within [-12, 12]", (double)semitones);
    if (step) *step = s;
    if (cutoff) *cutoff = c;
    if (half_taps) *half_taps = Kh;
    return VITS_OK;
}

int vits_warp_plan_rate(const int64_t *durations, const float *semitones, int len, int hop, int64_t L, int64_t M, vits_warp_seg *segs,
                        int64_t *spans, int64_t *n_out) {
    if (len < 0 || hop < 1 || (len > 0 && !durations)) return fail(nullptr, VITS_E_ARG, "bad warp plan arguments (len = %d, hop = %d)", len, hop);
    if (int rc = rate_ratio_fault(L, M)) return rc;
    int64_t ns = 0, N = 0;
    const std::string e = warp_plan_rate(durations, semitones, len, hop, L, M, segs, spans, ns, N);
    if (!e.empty()) return fail(nullptr, VITS_E_ARG, "%s", e.c_str());
    if (n_out) *n_out = N;
    return (int)ns;
}

int vits_glide_plan_rate(const int64_t *durations, const float *st0, const float *st1, int len, int hop, int64_t L, int64_t M,
                         vits_glide_seg *segs, int64_t *spans, int64_t *n_out) {
    if (len < 0 || hop < 1 || (len > 0 && !durations)) return fail(nullptr, VITS_E_ARG, "bad glide plan arguments (len = %d, hop = %d)", len, hop);
    if (int rc = rate_ratio_fault(L, M)) return rc;
    int64_t ns = 0, N = 0;
    const std::string e = glide_plan_rate(durations, st0, st1, len, hop, L, M, segs, spans, ns, N);
    if (!e.empty()) return fail(nullptr, VITS_E_ARG, "%s", e.c_str());
    if (n_out) *n_out = N;
    return (int)ns;
}

int vits_glide_cutoff_rate(int64_t step, int64_t *c, int32_t *half_taps) {
    if (step < kWarpRateMinStep || step > kWarpRateMaxStep)
        return fail(nullptr, VITS_E_ARG, "step %lld outside [%lld, %lld]", (long long)step, (long long)kWarpRateMinStep, (long long)kWarpRateMaxStep);
    int32_t c32, Kh;
    glide_cutoff(step, c32, Kh);
    if (c) *c = c32;
    if (half_taps) *half_taps = Kh;
    return VITS_OK;
}

int vits_glide_pos_rate(const vits_glide_seg *seg, int64_t j, int64_t *pos, int64_t *step) {
    if (!seg || !pos) return fail(nullptr, VITS_E_ARG, "null argument");
    vits_glide_seg g = *seg;
    g.n0 = 0;
    g.pos0 = 0;
    const std::string e = glide_rate_segs_fault(&g, 1);
    if (!e.empty()) return fail(nullptr, VITS_E_ARG, "%s", e.c_str());
    if (j < 0 || j > g.k) return fail(nullptr, VITS_E_ARG, "sample %lld outside [0, %lld]", (long long)j, (long long)g.k);
    *pos = glide_pos(seg->pos0, g.k, g.step0, g.step1, j);
    if (step) *step = glide_step(g.k, g.step0, g.step1, j < g.k ? j : g.k);
    return VITS_OK;
}

// the emit rule of a row of a folded plan and the cap, without a handle: half / min_step are the PLAN's largest Kh and least step
extern "C++" {
template <class Seg, class Fault>
static int rate_emit_end_as(const Seg *segs, int n_segs, int64_t n_in, int64_t n_out, int64_t X, int half, int64_t *ready, Fault fault) {
    if (n_segs < 1 || !segs || n_in < 0 || n_out < 0 || X < 0 || half < 1 || half > kWarpRateMaxHalf || !ready)
        return fail(nullptr, VITS_E_ARG, "bad emit end arguments (n_segs = %d, n_in = %lld, n_out = %lld, X = %lld, half = %d)", n_segs,
                    (long long)n_in, (long long)n_out, (long long)X, half);
    const std::string e = fault(segs, n_segs);
    if (!e.empty()) return fail(nullptr, VITS_E_ARG, "%s", e.c_str());
    const int64_t N = segs[n_segs - 1].n0 + segs[n_segs - 1].k;
    if (n_out != N) return fail(nullptr, VITS_E_ARG, "n_out = %lld, the row's records give %lld", (long long)n_out, (long long)N);
    *ready = warp_emit_row(segs, n_segs, n_in, n_out, X, half);
    return VITS_OK;
}
}  // extern "C++"

int vits_warp_emit_end_rate(const vits_warp_seg *segs, int n_segs, int64_t n_in, int64_t n_out, int64_t X, int half, int64_t *ready) {
    return rate_emit_end_as(segs, n_segs, n_in, n_out, X, half, ready, warp_rate_segs_fault);
}

int vits_glide_emit_end_rate(const vits_glide_seg *segs, int n_segs, int64_t n_in, int64_t n_out, int64_t X, int half, int64_t *ready) {
    return rate_emit_end_as(segs, n_segs, n_in, n_out, X, half, ready, glide_rate_segs_fault);
}

int vits_identity_emit_end_rate(int64_t L, int64_t M, int64_t K, int64_t n_in, int64_t X, int64_t *ready) {
    if (L < 1 || M < 1 || K < 0 || n_in < 0 || X < 0 || !ready)
        return fail(nullptr, VITS_E_ARG, "bad emit end arguments (L = %lld, M = %lld, K = %lld, n_in = %lld, X = %lld)", (long long)L, (long long)M,
                    (long long)K, (long long)n_in, (long long)X);
    WarpRateRow r{};
    r.L = L;
    r.M = M;
    r.K = (int32_t)K;
    r.n_out = (int32_t)((n_in * L + M - 1) / M);
    *ready = X >= n_in ? (int64_t)r.n_out : warp_rate_identity_ready(r, X);
    return VITS_OK;
}

int64_t vits_warp_stream_cap_rate(int64_t piece_samples, int64_t S_w, int64_t min_step, int half) {
    if (piece_samples < 1 || S_w < 1 || min_step < kWarpRateMinStep || min_step > kWarpRateMaxStep || half < 1 || half > kWarpRateMaxHalf)
        return fail(nullptr, VITS_E_ARG, "bad stream cap arguments (%lld, %lld, %lld, %d)", (long long)piece_samples, (long long)S_w,
                    (long long)min_step, half);
    return warp_stream_cap(piece_samples, S_w, min_step, half);
}

int vits_rate_identity_spans(const int64_t *durations, int len, int hop, int64_t L, int64_t M, int64_t n_in, int64_t *spans, int64_t *n_out) {
    if (len < 0 || hop < 1 || (len > 0 && !durations) || L < 1 || M < 1 || n_in < 0)
        return fail(nullptr, VITS_E_ARG, "bad identity row arguments (len = %d, hop = %d, L = %lld, M = %lld, n_in = %lld)", len, hop, (long long)L,
                    (long long)M, (long long)n_in);
    const int64_t N = warp_rate_identity(durations, len, hop, L, M, n_in, spans);
    if (n_out) *n_out = N;
    return VITS_OK;
}

void vits_free_output(vits_handle *h, vits_output *out) {
    if (!out) return;
    std::unique_lock<std::mutex> lk;
    if (h) lk = std::unique_lock<std::mutex>(h->mu);
    pinned_put(h, out->data);  // y_lengths lives in the same block
    out->data = nullptr;
    out->y_lengths = nullptr;
}

int vits_last_pcm16(vits_handle *h, int normalize, float volume, int16_t *out, size_t out_elems) {
    if (int rc = check_dev(h)) return rc;
    std::lock_guard<std::mutex> lk(h->mu);
    const int B = h->B, S = h->S;
    if (!h->d_out || !h->d_ylen || B <= 0 || S <= 0) return fail(h, VITS_E_ARG, "no completed run to post-process");
    const size_t n = (size_t)B * S;
    if (!out || out_elems < n) return fail(h, VITS_E_ARG, "pcm16 buffer too small: %zu < %zu", out_elems, n);
    // the staging slab is idle between runs (vits_run has consumed its inputs before it returns)
    PcmBufs pb;
    const bool rs = h->out_resampled;  // the waveform is the resampled one: its walk carved these buffers behind it
    if (rs) {
        const int K = h->rs_run_K;
        if (int rc = slab_carve(h, h->io, "staging", [&](Carver &cv) { pb = carve_resample(cv, B, S, K).pcm; })) return rc;
        if (!h->d_out) return fail(h, VITS_E_ARG, "no completed run to post-process");
    } else if (int rc = slab_carve(h, h->io, "staging", [&](Carver &cv) { pb = carve_pcm16(cv, B, S); }))
        return rc;
    int16_t *d_pcm = pb.pcm;
    unsigned *d_peak = pb.peak;
    hipStream_t st = h->stream;
    hipError_t e = hipMemsetAsync(d_peak, 0, (size_t)B * 4, st);
    // (valid samples of a row: y_len[b] * hop, or - resampled - its output sample count)
    const int hop = rs ? 1 : h->model.hop;
    const int *vlen = rs ? h->d_nout : h->d_ylen;
    if (e == hipSuccess) {
        int gx = (S + 255) / 256;
        gx = gx > 256 ? 256 : gx;
        peak_abs_kernel<<<dim3(gx, B), 256, 0, st>>>(h->d_out, vlen, hop, S, d_peak);
        pcm16_kernel<<<dim3((S + 255) / 256, B), 256, 0, st>>>(h->d_out, vlen, hop, S, d_peak, normalize, volume, d_pcm);
        e = hipGetLastError();
    }
    if (e == hipSuccess) e = hipMemcpyAsync(out, d_pcm, n * 2, hipMemcpyDeviceToHost, st);
    if (e == hipSuccess) e = hipStreamSynchronize(st);
    if (e != hipSuccess) return fail(h, VITS_E_DEVICE, "pcm16 post-processing failed: %s", hipGetErrorString(e));
    if (int rc = range_check(h)) return rc;  // (after vits_run_async this is the first synchronisation of that run)
    if (h->range_failed) return fail(h, VITS_E_RANGE, "the last run left the range of the fp16 operand planes (see vits_get_stats)");
    return VITS_OK;
}

// ---- delivery (vitsmi.h, "delivery"): the plan on the host (delivery.hpp), two launches (delivery.hip.hpp), one copy per
// silence-free run of segments, the silence filled in here while the copies run

// the layout of a plan over counts [B] (the rows' valid samples, or what is kept of them), with the trims' and the levels'
// validation where they are given: the three plan exports
static int plan_layout(const int64_t *counts, int B, const vits_segment *segs, const vits_trim *trims, const vits_level *levels, int n_segs,
                       int n_streams, int encoding, int sample_rate, int64_t *stream_samples, int64_t *stream_offsets,
                       int64_t *total_bytes) {
    DeliveryPlan p;
    std::string e = delivery_plan(counts, B, 0, segs, n_segs, n_streams, encoding, p, trims);
    if (e.empty()) e = level_plan_fault(segs, levels, n_segs, n_streams, sample_rate);
    if (!e.empty()) return fail(nullptr, VITS_E_ARG, "%s", e.c_str());
    for (int j = 0; j < n_streams && stream_samples; j++) stream_samples[j] = p.stream_samples[j];
    for (int j = 0; j <= n_streams && stream_offsets; j++) stream_offsets[j] = p.stream_offsets[j];
    if (total_bytes) *total_bytes = p.total_bytes;
    return VITS_OK;
}

int vits_delivery_plan(const int64_t *counts, int B, const vits_segment *segs, int n_segs, int n_streams, int encoding,
                       int64_t *stream_samples, int64_t *stream_offsets, int64_t *total_bytes) {
    return plan_layout(counts, B, segs, nullptr, nullptr, n_segs, n_streams, encoding, 0, stream_samples, stream_offsets, total_bytes);
}

int vits_trim_range(int64_t n, int64_t first_active, int64_t last_active, const vits_trim *t, int64_t *a, int64_t *c) {
    if (!t || !a || !c) return fail(nullptr, VITS_E_ARG, "null argument");
    const std::string e = trim_fault(*t);
    if (!e.empty()) return fail(nullptr, VITS_E_ARG, "%s", e.c_str());
    if (n < 0 || n > INT_MAX) return fail(nullptr, VITS_E_ARG, "n = %lld outside [0, %d]", (long long)n, INT_MAX);
    if (first_active <= last_active && (first_active < 0 || last_active >= n))
        return fail(nullptr, VITS_E_ARG, "active samples [%lld, %lld] outside [0, %lld)", (long long)first_active, (long long)last_active, (long long)n);
    trim_range(n, first_active, last_active, *t, *a, *c);
    return VITS_OK;
}

int vits_delivery_plan_trimmed(const int64_t *kept, int B, const vits_segment *segs, const vits_trim *trims, int n_segs, int n_streams,
                               int encoding, int64_t *stream_samples, int64_t *stream_offsets, int64_t *total_bytes) {
    return plan_layout(kept, B, segs, trims, nullptr, n_segs, n_streams, encoding, 0, stream_samples, stream_offsets, total_bytes);
}

int vits_loudness_filter(int sample_rate, double *coef, int32_t *hop) {
    if (sample_rate < kLevelMinRate || sample_rate > kLevelMaxRate)
        return fail(nullptr, VITS_E_ARG, "sample_rate %d outside [%d, %d]", sample_rate, kLevelMinRate, kLevelMaxRate);
    if (coef) loudness_filter(sample_rate, coef);
    if (hop) *hop = loudness_hop(sample_rate);
    return VITS_OK;
}

int vits_loudness_gate(const float *e, const int32_t *n_sub, int n_rows, int32_t hop, double *L, int32_t *n_blocks, int32_t *n_abs,
                       int32_t *n_rel) {
    if (n_rows < 0 || (n_rows > 0 && !n_sub) || hop < 1) return fail(nullptr, VITS_E_ARG, "loudness gate: n_rows = %d, hop = %d", n_rows, hop);
    size_t total = 0;
    for (int r = 0; r < n_rows; r++) {
        if (n_sub[r] < 0) return fail(nullptr, VITS_E_ARG, "loudness gate: n_sub[%d] = %d is negative", r, n_sub[r]);
        total += (size_t)n_sub[r];
    }
    if (total > 0 && !e) return fail(nullptr, VITS_E_ARG, "null argument");
    const LoudGate g = loudness_gate(e, n_sub, n_rows, hop);
    if (L) *L = g.L;
    if (n_blocks) *n_blocks = g.blocks;
    if (n_abs) *n_abs = g.abs_pass;
    if (n_rel) *n_rel = g.rel_pass;
    return VITS_OK;
}

int vits_level_gain(double L, float peak, const vits_level *level, float *gain) {
    if (!level || !gain) return fail(nullptr, VITS_E_ARG, "null argument");
    const std::string e = level_fault(*level);
    if (!e.empty()) return fail(nullptr, VITS_E_ARG, "%s", e.c_str());
    if (std::isnan(L) || L == std::numeric_limits<double>::infinity() || !(peak >= 0.f))
        return fail(nullptr, VITS_E_ARG, "loudness %g / peak %g: a loudness is a number or -inf, a peak is >= 0", L, (double)peak);
    *gain = level_gain(L, peak, *level);
    return VITS_OK;
}

int vits_delivery_plan_leveled(const int64_t *kept, int B, const vits_segment *segs, const vits_trim *trims, const vits_level *levels,
                               int n_segs, int n_streams, int encoding, int sample_rate, int64_t *stream_samples,
                               int64_t *stream_offsets, int64_t *total_bytes) {
    return plan_layout(kept, B, segs, trims, levels, n_segs, n_streams, encoding, sample_rate, stream_samples, stream_offsets, total_bytes);
}

int vits_shape_check(const vits_shape *shapes, int n_segs, const vits_env_point *points, int64_t n_points) {
    if (n_segs < 0) return fail(nullptr, VITS_E_ARG, "n_segs = %d is negative", n_segs);
    const std::string e = shape_fault(shapes, n_segs, points, n_points);
    if (!e.empty()) return fail(nullptr, VITS_E_ARG, "%s", e.c_str());
    return VITS_OK;
}

int vits_shape_gain(const vits_shape *shape, const vits_env_point *points, int64_t a, int64_t c, int64_t i, float *mul) {
    if (!shape || !mul) return fail(nullptr, VITS_E_ARG, "null argument");
    if (shape->first_point < 0 || shape->n_points < 0 || shape->first_point > kShapeMaxPoints - shape->n_points)
        return fail(nullptr, VITS_E_ARG, "points [%lld, +%d) outside [0, %lld]", (long long)shape->first_point, shape->n_points,
                    (long long)kShapeMaxPoints);
    const std::string e = shape_fault(shape, 1, points, shape->first_point + shape->n_points);
    if (!e.empty()) return fail(nullptr, VITS_E_ARG, "%s", e.c_str());
    if (a < 0 || c < 0 || a > INT_MAX - c || i < a || i >= a + c)
        return fail(nullptr, VITS_E_ARG, "sample %lld outside the kept range [%lld, +%lld) of a row of at most %d samples", (long long)i,
                    (long long)a, (long long)c, INT_MAX);
    std::vector<float> slopes;
    shape_slopes(points, shape->first_point + shape->n_points, slopes);
    const ShapeSeg t{(int32_t)a, (int32_t)c, shape->fade_in, shape->fade_out, shape->curve, shape->n_points, shape->first_point};
    *mul = shape_gain(t, points, slopes.data(), (int32_t)i);
    return VITS_OK;
}

// the valid samples of the rows of a run that can be delivered: frames * hop, or their count at the rate the run was
// resampled to
static int delivery_counts(vits_handle *h, std::vector<int64_t> &counts) {
    const int B = h->B, S = h->S;
    counts.resize(B);
    for (int b = 0; b < B; b++) {
        const int64_t n = (int64_t)(h->last_vocoder ? h->F : h->h_ylen[b]) * h->model.hop;
        if ((int)h->warp_counts.size() == B) counts[b] = h->warp_counts[b];  // (a warped run: its plan's)
        else if ((int)h->run_L.size() == B) counts[b] = (n * h->run_L[b] + h->run_M[b] - 1) / h->run_M[b];  // (a rate per row)
        else counts[b] = h->out_resampled ? (n * h->rs_run_L + h->rs_run_M - 1) / h->rs_run_M : n;
        if (counts[b] > S) return fail(h, VITS_E_ARG, "no completed run to deliver (row %d: %lld samples of %d)", b, (long long)counts[b], S);
    }
    return 0;
}

// The handle's side of every delivery (the sequence: delivery_run.hip.hpp): the last run's waveform and its rows' valid
// samples, the call's buffers from the staging slab, the range check behind the call's first wait.
static int deliver_last_run(vits_handle *h, const DeliveryRequest &rq, const DeliveryOutputs &out) {
    if (int rc = check_dev(h)) return rc;
    std::lock_guard<std::mutex> lk(h->mu);
    const int B = h->B, S = h->S;
    if (!h->d_out || B <= 0 || S <= 0 || (!h->last_vocoder && (int)h->h_ylen.size() != B))
        return fail(h, VITS_E_ARG, "no completed run to deliver");
    std::vector<int64_t> counts;
    if (int rc = delivery_counts(h, counts)) return rc;
    auto bufs = [&](const DeliveryNeeds &need, const float *&d_x, DeliveryCallBufs &cb) -> DeliveryStatus {
        if (need.levelled && h->rs.plan.on() && rq.sample_rate != h->rs.plan.fo)
            return delivery_refusal(VITS_E_ARG, "sample_rate %d differs from the output rate %d", rq.sample_rate, (int)h->rs.plan.fo);
        // (a run with a rate per row: the loudness filter of a call is one rate's, so every levelled segment's row must be at it)
        for (int g = 0; need.levelled && (int)h->run_rates.size() == B && g < rq.n_segs; g++)
            if (rq.levels[g].mode != 0 && h->run_rates[rq.segs[g].row] != rq.sample_rate)
                return delivery_refusal(VITS_E_ARG, "segment %d: sample_rate %d differs from the rate %d its row %d was delivered at", g,
                                        rq.sample_rate, (int)h->run_rates[rq.segs[g].row], (int)rq.segs[g].row);
        // the staging slab is idle between runs; a resampled waveform lives in it, and its walk carved these buffers behind it
        if (h->out_resampled) {
            // (the run's own walk ends with carve_resample, or with an encoded stream's buffers behind it; the trim slots behind
            // carve_resample are at most 12 B + 512 bytes more than the former.  Growing the slab here would drop the waveform that
            // lives in it - the check below - and does not happen: slab_reserve allocates 1 MiB above every request, and
            // vits_reserve counts this walk.  A levelled delivery's buffers - some 0.05 bytes a sample - fit into the quarter a
            // growing slab adds to every request; where a slab does not hold them the call is refused and the run stays
            // deliverable.)
            const int K = h->rs_run_K;
            auto walk = [&](Carver &cv) {
                const DeliveryBufs front = carve_resample(cv, B, S, K).dlv;
                cb = carve_delivery_call(cv, B, S, need, &front);
            };
            if ((need.levelled || need.shaped) && carved_bytes(walk) > h->io.cap)
                return delivery_refusal(VITS_E_NOMEM,
                                        "a levelled, shaped or limited delivery of this run needs %zu bytes of staging, %zu are there: vits_reserve covers it",
                                        carved_bytes(walk), h->io.cap);
            if (int rc = slab_carve(h, h->io, "staging", walk)) return {rc, h->err};
            if (!h->d_out) return delivery_refusal(VITS_E_ARG, "no completed run to deliver");
        } else if (int rc = slab_carve(h, h->io, "staging", [&](Carver &cv) { cb = carve_delivery_call(cv, B, S, need); }))
            return {rc, h->err};
        d_x = h->d_out;
        return {};
    };
    auto waited = [&]() -> DeliveryStatus {  // (after vits_run_async this is the first synchronisation of that run)
        if (int rc = range_check(h)) return {rc, h->err};
        if (h->range_failed)
            return delivery_refusal(VITS_E_RANGE, "the last run left the range of the fp16 operand planes (see vits_get_stats)");
        return {};
    };
    const DeliveryStatus s = delivery_run(counts.data(), B, S, h->stream, rq, out, bufs, waited);
    return s.code ? fail(h, s.code, "%s", s.msg.c_str()) : VITS_OK;
}

int vits_deliver(vits_handle *h, const vits_segment *segs, int n_segs, int n_streams, int encoding, void *dst, size_t dst_bytes,
                 int64_t *stream_samples, int64_t *stream_offsets) {
    return deliver_last_run(h, {segs, nullptr, nullptr, nullptr, nullptr, 0, n_segs, n_streams, encoding, 0, dst, dst_bytes, /*kept=*/false},
                            {stream_samples, stream_offsets, nullptr, nullptr, nullptr, nullptr});
}

// vits_deliver_trimmed, vits_deliver_leveled and vits_deliver_shaped: levels == nullptr is the first exactly, shapes == nullptr
// (or shapes without fades and points) the second
int vits_deliver_trimmed(vits_handle *h, const vits_segment *segs, const vits_trim *trims, int n_segs, int n_streams, int encoding,
                         void *dst, size_t dst_bytes, int64_t *stream_samples, int64_t *stream_offsets, int64_t *kept_first,
                         int64_t *kept_count) {
    return deliver_last_run(h, {segs, trims, nullptr, nullptr, nullptr, 0, n_segs, n_streams, encoding, 0, dst, dst_bytes, /*kept=*/true},
                            {stream_samples, stream_offsets, kept_first, kept_count, nullptr, nullptr});
}

int vits_deliver_leveled(vits_handle *h, const vits_segment *segs, const vits_trim *trims, const vits_level *levels, int n_segs,
                         int n_streams, int encoding, int sample_rate, void *dst, size_t dst_bytes, int64_t *stream_samples,
                         int64_t *stream_offsets, int64_t *kept_first, int64_t *kept_count, double *loudness, float *gain) {
    return deliver_last_run(h, {segs, trims, levels, nullptr, nullptr, 0, n_segs, n_streams, encoding, sample_rate, dst, dst_bytes, /*kept=*/true},
                            {stream_samples, stream_offsets, kept_first, kept_count, loudness, gain});
}

int vits_deliver_shaped(vits_handle *h, const vits_segment *segs, const vits_trim *trims, const vits_level *levels,
                        const vits_shape *shapes, const vits_env_point *points, int64_t n_points, int n_segs, int n_streams,
                        int encoding, int sample_rate, void *dst, size_t dst_bytes, int64_t *stream_samples, int64_t *stream_offsets,
                        int64_t *kept_first, int64_t *kept_count, double *loudness, float *gain) {
    return deliver_last_run(h, {segs, trims, levels, shapes, points, n_points, n_segs, n_streams, encoding, sample_rate, dst, dst_bytes, /*kept=*/true},
                            {stream_samples, stream_offsets, kept_first, kept_count, loudness, gain});
}

// vits_deliver_limited: limits == nullptr (or every mode 0) is vits_deliver_shaped exactly
int vits_limit_check(const vits_limit *limits, const vits_segment *segs, int n_segs) {
    if (n_segs < 0) return fail(nullptr, VITS_E_ARG, "n_segs = %d is negative", n_segs);
    const std::string e = limit_fault(limits, segs, n_segs);
    if (!e.empty()) return fail(nullptr, VITS_E_ARG, "%s", e.c_str());
    return VITS_OK;
}

int vits_limit_gains(const float *u, int64_t c, const vits_limit *limit, float *g) {
    if (!limit || c < 0 || c > INT_MAX || (c > 0 && (!u || !g))) return fail(nullptr, VITS_E_ARG, "bad limiter arguments (c = %lld)", (long long)c);
    const std::string e = limit_fault(limit, nullptr, 1);
    if (!e.empty()) return fail(nullptr, VITS_E_ARG, "%s", e.c_str());
    if (limit->mode == 0) std::fill(g, g + c, 1.0f);
    else limit_gains(u, c, limit->ceiling, limit->lookahead, g);
    return VITS_OK;
}

int vits_deliver_limited(vits_handle *h, const vits_segment *segs, const vits_trim *trims, const vits_level *levels,
                         const vits_shape *shapes, const vits_env_point *points, int64_t n_points, const vits_limit *limits, int n_segs,
                         int n_streams, int encoding, int sample_rate, void *dst, size_t dst_bytes, int64_t *stream_samples,
                         int64_t *stream_offsets, int64_t *kept_first, int64_t *kept_count, double *loudness, float *gain) {
    return deliver_last_run(h, {segs, trims, levels, shapes, points, n_points, n_segs, n_streams, encoding, sample_rate, dst, dst_bytes, /*kept=*/true, limits},
                            {stream_samples, stream_offsets, kept_first, kept_count, loudness, gain});
}

// vocoder-only entry points: z (host, [B, inter, F], already masked) -> device, speaker bias; then either the whole
// waveform or chunks
static int vocoder_common(vits_handle *h, const float *z, int B, int F, const int64_t *sid, vits_output *out,
                          const ChunkSink *sink) {
    const Model &m = h->model;
    if (!z || (!out && !sink) || B <= 0 || F <= 0) return fail(h, VITS_E_ARG, "bad vocoder arguments");
    if (int rc = row_rates_admit(h, B, sink ? "a chunked vocoder run" : nullptr)) return rc;
    if (m.gin && !sid) return fail(h, VITS_E_ARG, "Missing speaker id");
    for (int b = 0; sid && m.gin && b < B; b++)
        if (sid[b] < 0 || sid[b] >= m.n_speakers)
            return fail(h, VITS_E_ARG, "sid[%d]=%lld is out of range [0,%d)", b, (long long)sid[b], m.n_speakers);
    std::memset(&h->stats, 0, sizeof h->stats);
    h->conv_events_used = 0;
    g_launch_name_on = h->timing == 1;
    h->range_failed = false;
    const size_t nCF = (size_t)B * m.C * F;
    const int Fgen = gen_frames(m, F, sink ? sink->chunk_frames : 0);
    FrameBufs fb;
    if (int rc = slab_carve(h, h->frm, "frame", [&](Carver &cv) { fb = carve_frames(cv, m, B, F, Fgen, /*flow=*/false); })) return rc;
    hipStream_t st = h->stream;
    float *dz = fb.voc.z;
    HIPCHECK(h, hipMemcpyAsync(dz, z, nCF * 4, hipMemcpyHostToDevice, st));
    Ctx c{h, m, st, h->arena_dev, B};
    float *dec_cond = nullptr;
    int64_t *d_sid = nullptr;
    if (m.gin) {
        d_sid = fb.voc.sid;
        HIPCHECK(h, hipMemcpyAsync(d_sid, sid, (size_t)B * 8, hipMemcpyHostToDevice, st));
        dec_cond = fb.voc.dec_cond;
        cond_matvec_kernel<<<dim3((m.C0 + 63) / 64, B), 64, 0, st>>>(c.P(m.emb_g), d_sid, m.n_speakers, c.P(m.dec_cond_w),
                                                                    c.P(m.dec_cond_b), dec_cond, m.C0, m.gin);
    }
    h->B = B;
    h->F = F;
    h->out_resampled = false;
    forget_row_run(h);
    h->last_vocoder = true;
    h->d_ylen = nullptr;  // (no frame counts: vits_last_pcm16 does not apply to a vocoder-only run)
    h->h_dur_B = h->h_dur_T = 0;  // (no tokens: vits_last_durations has nothing to report)
    range_begin(h);
    int rc;
    if (sink) rc = render_chunks(h, c, dz, (int64_t)m.C * F, F, nullptr, B, F, dec_cond, fb, Fgen, *sink);
    else rc = run_generator(h, c, dz, (int64_t)m.C * F, F, nullptr, B, F, dec_cond, fb.gen);
    if (rc) return rc;
    if (c.err != hipSuccess) return fail(h, VITS_E_DEVICE, "kernel launch failed: %s", hipGetErrorString(c.err));
    if (h->rs.plan.on() && !sink)
        if (int rc2 = resample_run(h, nullptr, B)) return rc2;
    if (h->rows.on() && !sink)
        if (int rc2 = resample_rows_run(h, nullptr, B)) return rc2;
    range_end(h);
    if (sink) {
        HIPCHECK(h, hipStreamSynchronize(st));
        return range_check(h);
    }
    size_t n = (size_t)B * h->S;
    float *host = (float *)pinned_get(h, n * 4 + 64);
    if (!host) return fail(h, VITS_E_NOMEM, "pinned alloc failed");
    hipError_t ce = hipMemcpyAsync(host, h->d_out, n * 4, hipMemcpyDeviceToHost, st);
    if (ce == hipSuccess) ce = hipStreamSynchronize(st);
    if (ce != hipSuccess) {
        pinned_put(h, host);
        return fail(h, VITS_E_DEVICE, "device-to-host copy failed: %s", hipGetErrorString(ce));
    }
    if (int rr = range_check(h)) {
        pinned_put(h, host);
        return rr;
    }
    out->data = host;
    out->dims[0] = B;
    out->dims[1] = 1;
    out->dims[2] = 1;
    out->dims[3] = h->S;
    out->y_lengths = nullptr;
    return VITS_OK;
}

int vits_run_vocoder(vits_handle *h, const float *z, int B, int F, const int64_t *sid, vits_output *out) {
    if (int rc = check_dev(h)) return rc;
    std::lock_guard<std::mutex> lk(h->mu);
    if (!out) return fail(h, VITS_E_ARG, "bad vocoder arguments");
    return vocoder_common(h, z, B, F, sid, out, nullptr);
}

// the chunked vocoder entries, in the order of run_call_locked: the stream arguments of an encoded sink, then the device
static int run_vocoder_chunked(vits_handle *h, const float *z, int B, int F, const int64_t *sid, bool encoded, const ChunkSink &sink) {
    if (!h) return VITS_E_ARG;
    std::lock_guard<std::mutex> lk(h->mu);
    if (encoded)
        if (int rc = host_stream(h, sink, B)) return rc;
    if (int rc = check_dev(h)) return rc;
    if (sink.chunk_frames < 1) return fail(h, VITS_E_ARG, "bad vocoder arguments");
    return vocoder_common(h, z, B, F, sid, nullptr, &sink);
}

int vits_run_vocoder_chunked(vits_handle *h, const float *z, int B, int F, const int64_t *sid, int chunk_frames,
                             vits_chunk_fn fn, void *user) {
    return run_vocoder_chunked(h, z, B, F, sid, false, ChunkSink{chunk_frames, fn, user});
}

int vits_run_vocoder_chunked_enc_trimmed(vits_handle *h, const float *z, int B, int F, const int64_t *sid, const vits_stream_format *fmt,
                                         const vits_stream_shaping *shaping, const vits_stream_onset *onsets, int chunk_frames,
                                         vits_enc_chunk_trim_fn fn, void *user) {
    return run_vocoder_chunked(h, z, B, F, sid, true, encoded_sink(chunk_frames, fmt, shaping, onsets, nullptr, fn, user));
}

int vits_run_vocoder_chunked_enc_shaped(vits_handle *h, const float *z, int B, int F, const int64_t *sid, const vits_stream_format *fmt,
                                        const vits_stream_shaping *shaping, int chunk_frames, vits_enc_chunk_fn fn, void *user) {
    return run_vocoder_chunked(h, z, B, F, sid, true, encoded_sink(chunk_frames, fmt, shaping, nullptr, fn, nullptr, user));
}

int vits_run_vocoder_chunked_enc(vits_handle *h, const float *z, int B, int F, const int64_t *sid, const vits_stream_format *fmt,
                                 int chunk_frames, vits_enc_chunk_fn fn, void *user) {
    return vits_run_vocoder_chunked_enc_shaped(h, z, B, F, sid, fmt, nullptr, chunk_frames, fn, user);
}

int vits_tap(vits_handle *h, const char *name, float *buf, size_t buf_elems, int64_t dims[VITS_MAX_DIMS]) {
    if (int rc = check_dev(h)) return rc;
    std::lock_guard<std::mutex> lk(h->mu);
    if (!name || !dims) return fail(h, VITS_E_ARG, "null argument");
    const Model &m = h->model;
    const int B = h->B, T = h->T, F = h->F;
    std::string k = name;
    const float *src = nullptr;
    int64_t bstride = 0;
    int nd = 3, C = 0, L = 0, cstride = 0;
    if (k == "x") { src = h->d_x; C = m.H; L = T; bstride = (int64_t)C * L; }
    else if (k == "emb") { src = h->d_emb; C = m.H; L = T; bstride = (int64_t)C * L; }
    else if (k == "m_p") { src = h->d_mp; C = m.C; L = T; bstride = (int64_t)2 * C * L; }
    else if (k == "logs_p") { src = h->d_logs; C = m.C; L = T; bstride = (int64_t)2 * C * L; }
    else if (k == "logw") { src = h->d_logw; C = 1; L = T; bstride = L; }
    else if (k == "w_ceil") { src = h->d_wceil; C = 1; L = T; bstride = L; nd = 2; }
    else if (k == "w") { src = h->d_fit_w; C = 1; L = T; bstride = L; nd = 2; }
    else if (k == "z_p") { src = h->d_zp; C = m.C; L = F; cstride = h->Fpitch; bstride = (int64_t)C * cstride; }
    else if (k == "z") { src = h->d_z; C = m.C; L = F; cstride = h->Fpitch; bstride = (int64_t)C * cstride; }
    else return fail(h, VITS_E_ARG, "unknown tap %s", name);
    if (k == "logw" && h->last_forced && h->d_wceil)
        return fail(h, VITS_E_ARG, "logw is not computed in a forced-duration run");
    if (k == "w" && !src && h->d_wceil) return fail(h, VITS_E_ARG, "w is not computed in a run without a fit");
    if (!src || B == 0) return fail(h, VITS_E_ARG, "no completed run to tap");
    if (nd == 2) { dims[0] = B; dims[1] = L; }
    else { dims[0] = B; dims[1] = C; dims[2] = L; }
    size_t n = (size_t)B * C * L;
    if (!buf) return nd;
    if (buf_elems < n) return fail(h, VITS_E_ARG, "tap buffer too small: %zu < %zu", buf_elems, n);
    float *tmp = nullptr;
    HIPCHECK(h, hipMalloc((void **)&tmp, n * 4 + 16));
    gather_view_kernel<<<dim3((L + 255) / 256, C, B), 256, 0, h->stream>>>(src, bstride, cstride ? cstride : L, tmp, C, L);
    hipError_t e = hipMemcpyAsync(buf, tmp, n * 4, hipMemcpyDeviceToHost, h->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(h->stream);
    hipFree(tmp);
    if (e != hipSuccess) return fail(h, VITS_E_DEVICE, "tap copy failed: %s", hipGetErrorString(e));
    return nd;
}

int vits_get_stats(vits_handle *h, vits_stats *out) {
    if (!h || !out) return VITS_E_ARG;
    if (!h->host_only) {
        hipSetDevice(h->device);
        hipStreamSynchronize(h->stream);
        range_check(h);  // fills stats.f16_*; a violation stays on record for vits_sync (range_failed)
        if (h->timing) {
            float ms = 0.f, tot = 0.f, tot_sx = 0.f;
            for (size_t i = 0; i < h->conv_events_used; i++) {
                if (hipEventElapsedTime(&ms, h->conv_events[i].first, h->conv_events[i].second) != hipSuccess) continue;
                h->conv_recs[i].ms = ms;
                tot += ms;
                if (i < h->conv_event_sx.size() && h->conv_event_sx[i]) tot_sx += ms;
            }
            h->stats.conv_ms = tot;
            h->stats.sx_ms = tot_sx;
            auto el = [&](int a, int b) {
                float v = 0.f;
                if (hipEventElapsedTime(&v, h->ev[a], h->ev[b]) != hipSuccess) v = 0.f;
                return v;
            };
            h->stats.enc_ms = el(0, 1);
            h->stats.dp_ms = el(1, 2);
            h->stats.flow_ms = el(2, 3);
            h->stats.dec_ms = el(3, 4);
            h->stats.total_ms = el(0, 4);
        }
    }
    *out = h->stats;
    return VITS_OK;
}

int vits_launch_records(vits_handle *h, vits_launch_record *buf, int n) {
    if (!h) return VITS_E_ARG;
    std::lock_guard<std::mutex> lk(h->mu);
    const int have = (int)h->conv_events_used;
    for (int i = 0; i < have && i < n && buf; i++) buf[i] = h->conv_recs[i];
    return have;
}

void *vits_host_alloc(size_t bytes) {
    void *p = nullptr;
    return hipHostMalloc(&p, bytes ? bytes : 1) == hipSuccess ? p : nullptr;
}

void vits_host_free(void *p) {
    if (p) hipHostFree(p);
}

int vits_fetch_output(vits_handle *h, float *dst, size_t row_elems, size_t dst_elems) {
    if (int rc = check_dev(h)) return rc;
    std::lock_guard<std::mutex> lk(h->mu);
    const int B = h->B, S = h->S;
    if (!h->d_out || B <= 0 || S <= 0) return fail(h, VITS_E_ARG, "no completed run to fetch");
    if (!dst || row_elems < (size_t)S || dst_elems < (size_t)B * row_elems)
        return fail(h, VITS_E_ARG, "output buffer too small: rows of %zu (need %d), %zu elements (need %zu)", row_elems, S,
                    dst_elems, (size_t)B * row_elems);
    hipStream_t st = h->stream;
    hipError_t e = row_elems == (size_t)S
                       ? hipMemcpyAsync(dst, h->d_out, (size_t)B * S * 4, hipMemcpyDeviceToHost, st)
                       : hipMemcpy2DAsync(dst, row_elems * 4, h->d_out, (size_t)S * 4, (size_t)S * 4, B, hipMemcpyDeviceToHost, st);
    if (row_elems > (size_t)S)  // (host work while the copy runs: the tail columns belong to nobody else)
        for (int b = 0; b < B; b++) std::memset(dst + (size_t)b * row_elems + S, 0, (row_elems - S) * 4);
    if (e == hipSuccess) e = hipStreamSynchronize(st);
    if (e != hipSuccess) return fail(h, VITS_E_DEVICE, "device-to-host copy failed: %s", hipGetErrorString(e));
    if (int rc = range_check(h)) return rc;
    if (h->range_failed) return fail(h, VITS_E_RANGE, "the last run left the range of the fp16 operand planes (see vits_get_stats)");
    return VITS_OK;
}

// ---------------------------------------------------------------- kernel-level test hooks

static int test_dev(int device_id) {
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess || device_id < 0 || device_id >= n)
        return fail(nullptr, VITS_E_DEVICE, "no usable HIP device %d", device_id);
    if (hipSetDevice(device_id) != hipSuccess) return fail(nullptr, VITS_E_DEVICE, "hipSetDevice failed");
    return 0;
}

#define TCHECK(expr)                                                                                        \
    do {                                                                                                    \
        hipError_t _e = (expr);                                                                             \
        if (_e != hipSuccess) return fail(nullptr, VITS_E_DEVICE, "%s: %s", #expr, hipGetErrorString(_e)); \
    } while (0)

static int run_test_conv(const ConvDesc &d, const std::vector<float> &arena, const float *x, int B, int T,
                         int flags, float slope, float *out, size_t out_elems, int64_t out_bstride) {
    DevBufs D;
    const size_t nx = (size_t)B * d.Cin * T;
    float *dA = D.up(arena.data(), arena.size());
    float *dx = D.up(x, nx, 16);
    float *dout = D.fill<float>(out_elems, 0, 16);
    TCHECK(D.err);
    ConvArgs a = conv_args(d, dA, dA);  // (pack_test_* reserve a zero page at offset 0)
    a.x = dx;
    a.x_bstride = (int64_t)d.Cin * T;
    a.T = T;
    a.out = dout;
    a.out_bstride = out_bstride;
    a.flags = ((flags & 1) ? PRO_LRELU : 0) | ((flags & 2) ? EPI_RELU : 0);
    a.slope = slope;
    TCHECK(launch_conv(a, d.cfg, B, nullptr));
    TCHECK(hipDeviceSynchronize());
    TCHECK(download(out, dout, out_elems));
    return VITS_OK;
}

int vits_test_conv1d(int device_id, const float *x, int B, int Cin, int T, const float *w, const float *bias, int Cout,
                     int K, int dil, int pad_l, int flags, float slope, float *out) {
    if (int rc = test_dev(device_id)) return rc;
    ConvDesc d;
    std::vector<float> arena;
    { std::string e = pack_test_conv(w, bias, Cin, Cout, K, dil, pad_l, (flags >> 8) & 3, &d, &arena); if (!e.empty()) return fail(nullptr, VITS_E_ARG, "%s", e.c_str()); }
    return run_test_conv(d, arena, x, B, T, flags, slope, out, (size_t)B * Cout * T, (int64_t)Cout * T);
}

// the bench hooks' random data: one LCG stream, the weights (scaled by 0.05) first, then x
static void bench_fill(std::vector<float> &w, std::vector<float> &x) {
    uint32_t s = 12345u;
    auto rnd = [&]() {
        s = s * 1664525u + 1013904223u;
        return ((s >> 8) * (1.0f / 8388608.0f)) - 1.0f;
    };
    for (auto &v : w) v = rnd() * 0.05f;
    for (auto &v : x) v = rnd();
}

// Micro-benchmark of one conv shape on random data (kernel tuning; tools/conv_bench.py): returns the
// average launch time in ms over `iters` back-to-back launches (HIP events on the null stream).
int vits_bench_conv1d(int device_id, int B, int Cin, int Cout, int T, int K, int dil, int hint, int iters,
                      int cfg_override, int ck_override, float *ms_out) {
    if (int rc = test_dev(device_id)) return rc;
    std::vector<float> w((size_t)Cout * Cin * K), x((size_t)B * Cin * T);
    bench_fill(w, x);
    ConvDesc d;
    std::vector<float> arena;
    const int dbg = hint >> 8;  // bit0: no DMA after warm-up chunks, bit1: no epilogue, bit2: no lrelu prologue
    hint &= 3;
    TestPack o;
    o.cfg = cfg_override;
    o.ck = ck_override;
    std::string e = pack_test_conv(w.data(), nullptr, Cin, Cout, K, dil, dil * (K - 1) / 2, hint, &d, &arena, o);
    if (!e.empty()) return fail(nullptr, VITS_E_ARG, "%s", e.c_str());
    DevBufs D;
    float *dA = D.up(arena.data(), arena.size());
    float *dx = D.up(x.data(), x.size());
    float *dout = D.alloc<float>((size_t)B * Cout * T);
    TCHECK(D.err);
    ConvArgs a = conv_args(d, dA, dA);
    a.x = dx;
    a.x_bstride = (int64_t)Cin * T;
    a.T = T;
    a.out = dout;
    a.out_bstride = (int64_t)Cout * T;
    a.flags = ((dbg & 4) ? 0 : PRO_LRELU) | ((dbg & 1) ? DBG_NO_DMA : 0) | ((dbg & 2) ? DBG_NO_EPI : 0);
    if ((dbg & 8) && Cin == Cout) {  // residual epilogue + pre-activated second output, as the generator runs it
        a.flags |= EPI_RES;
        a.res = dx;
        a.res_bstride = (int64_t)Cin * T;
        a.oslope2 = 0.1f;
    }
    a.slope = 0.1f;
    auto go = [&] { return launch_conv(a, d.cfg, B, nullptr); };
    for (int i = 0; i < 2; i++) TCHECK(go());
    TCHECK(hipDeviceSynchronize());
    float ms = 0.f;
    TCHECK(time_launches(iters, go, &ms));
    if (ms_out) {
        ms_out[0] = ms;
        ms_out[1] = (float)d.cfg;
        ms_out[2] = (float)d.CK;
    }
    return VITS_OK;
}

int vits_test_conv_transpose1d(int device_id, const float *x, int B, int Cin, int T, const float *w, const float *bias,
                               int Cout, int K, int stride, float *out) {
    if (int rc = test_dev(device_id)) return rc;
    ConvDesc d;
    std::vector<float> arena;
    { std::string e = pack_test_convT(w, bias, Cin, Cout, K, stride, &d, &arena); if (!e.empty()) return fail(nullptr, VITS_E_ARG, "%s", e.c_str()); }
    return run_test_conv(d, arena, x, B, T, 0, 0.f, out, (size_t)B * Cout * T * stride, (int64_t)Cout * T * stride);
}

// The f32 engine with conv()'s whole argument set (include/vitsmi.h): conv_args() plus the field assignments conv() makes,
// one launch_conv().  Everything a launch could index out of its buffers with is refused here.
int vits_test_conv1d_epi(int device_id, vits_test_conv_epi_args *p) {
    if (int rc = test_dev(device_id)) return rc;
    if (!p) return fail(nullptr, VITS_E_ARG, "no arguments");
    const auto bad = [](const char *why) { return fail(nullptr, VITS_E_ARG, "conv epilogue hook: %s", why); };
    const int B = p->B, Cin = p->Cin, T = p->T, Cr = p->Cout, u = p->stride, flags = p->flags;
    if (B < 1 || Cin < 1 || T < 1 || Cr < 1 || u < 1 || !p->x || !p->w || !p->out) return bad("bad shape or missing tensor");
    if (flags & ~1023) return bad("unknown flag");
    const bool wn = flags & EPI_WN;
    if ((flags & EPI_WN_FIRST) && !wn) return bad("EPI_WN_FIRST without EPI_WN");
    if (wn && (flags & (EPI_RES | EPI_ACC | EPI_DIV | EPI_COUPLING))) return bad("EPI_WN excludes the other update rules");
    if (wn && !p->out2) return bad("EPI_WN needs out2 (the skip rows)");
    if (wn && (p->wn_split % 32 != 0 || p->wn_split < 0 || p->wn_split > Cr)) return bad("wn_split must be a multiple of 32 within Cout");
    if ((flags & EPI_RES) && !p->res) return bad("EPI_RES without res");
    if (p->bias_b && p->bias_b_stride < Cr) return bad("bias_b rows shorter than Cout");
    if (u > 1 && (wn || p->pl_rows || p->bias_b)) return bad("a transposed conv takes neither EPI_WN nor planes nor bias_b");
    const int planes_max = wn ? p->wn_split : Cr;
    if (p->pl_rows < 0 || p->pl_rows % 32 != 0 || p->pl_rows > planes_max) return bad("pl_rows must be a multiple of 32 within the rows stored in out");
    if (p->pl_rows && !p->planes_out) return bad("planes without planes_out");
    if (p->lens)
        for (int b = 0; b < B; b++)
            if (p->lens[b] < 0 || p->lens[b] > T) return bad("lens outside [0, T]");
    ConvDesc d;
    std::vector<float> arena;
    TestPack o;
    o.cfg = p->cfg >= 0 ? p->cfg : -1;
    o.ck = p->ck;
    if (p->cfg > 5 || (p->cfg >= 0 && p->ck != 8 && p->ck != 16 && p->ck != 32)) return bad("cfg 0..5 with a chunk of 8, 16 or 32 channels");
    if (u == 1 && (p->K < 1 || p->dil < 1 || p->pad_l < 0 || p->pad_l > (int64_t)p->dil * (p->K - 1))) return bad("pad_l outside the receptive field");
    {
        const std::string e = u > 1 ? pack_test_convT(p->w, p->bias, Cin, Cr, p->K, u, &d, &arena, false, o)
                                    : pack_test_conv(p->w, p->bias, Cin, Cr, p->K, p->dil, p->pad_l, p->hint & 3, &d, &arena, o);
        if (!e.empty()) return fail(nullptr, VITS_E_ARG, "%s", e.c_str());
    }
    const int Tout = T * u;
    const int xp = p->x_cstride ? p->x_cstride : T, op = p->out_cstride ? p->out_cstride : Tout;
    const int BN = conv_tile_n(d.cfg);
    if (xp < T) return bad("x_cstride smaller than T");
    if (u > 1 && op != Tout) return bad("a transposed conv stores dense rows (out_cstride = T * stride)");
    if (op < Tout) return bad("out_cstride smaller than T");
    if (u == 1 && op > (T + BN - 1) / BN * BN) return bad("out_cstride beyond the last time tile: nobody would zero those columns");
    const int rows = p->out_rows ? p->out_rows : Cr, row0 = p->out_row0;
    if (row0 < 0 || rows < 1) return bad("bad output window");
    if (wn ? (row0 != 0 || rows < p->wn_split || rows < Cr - p->wn_split) : row0 + Cr > rows) return bad("the conv's rows leave the output tensor");
    // host images: x with its pitch (zeros behind T), out / out2 with theirs (sentinel behind T and where nothing is old)
    std::vector<float> hx((size_t)B * Cin * xp, 0.f);
    for (size_t r = 0; r < (size_t)B * Cin; r++) std::memcpy(&hx[r * xp], p->x + r * T, (size_t)T * 4);
    const size_t no = (size_t)B * rows * op;
    const auto image = [&](const float *old) {
        std::vector<float> v(no, p->sentinel);
        if (old)
            for (size_t r = 0; r < (size_t)B * rows; r++) std::memcpy(&v[r * op], old + r * Tout, (size_t)Tout * 4);
        return v;
    };
    const std::vector<float> ho = image(p->old_out), ho2 = image(p->old_out2);
    std::vector<int> l32(B);
    for (int b = 0; b < B; b++) l32[b] = p->lens ? (int)p->lens[b] : T;
    const size_t npl = (size_t)B * (p->pl_rows ? p->pl_rows : 32) * T;
    DevBufs D;
    float *dA = D.up(arena.data(), arena.size());
    float *dx = D.up(hx.data(), hx.size(), 16);
    float *dout = D.up(ho.data(), no, 16);
    float *dout2 = p->out2 ? D.up(ho2.data(), no, 16) : nullptr;
    float *dres = p->res ? D.up(p->res, (size_t)B * Cr * op, 16) : nullptr;
    float *dbb = p->bias_b ? D.up(p->bias_b, (size_t)B * p->bias_b_stride) : nullptr;
    int *dlen = p->lens ? D.up(l32.data(), (size_t)B) : nullptr;
    uint16_t *dpl = D.fill<uint16_t>(npl * 3, 0x3c, 64);
    float *dpo = D.alloc<float>(npl, 16);
    TCHECK(D.err);
    ConvArgs a = conv_args(d, dA, dA);  // (pack_test_* reserve a zero page at offset 0)
    a.x = dx;
    a.x_bstride = (int64_t)Cin * xp;
    a.x_cstride = p->x_cstride;
    a.T = T;
    a.len = dlen;
    a.bias_b = dbb;
    a.bias_b_stride = p->bias_b_stride;
    a.out = dout + (size_t)row0 * op;
    a.out_bstride = (int64_t)rows * op;
    a.out_cstride = p->out_cstride;
    a.out2 = dout2 ? dout2 + (size_t)row0 * op : nullptr;
    a.res = dres;
    a.res_bstride = (int64_t)Cr * op;
    a.flags = flags;
    a.slope = p->slope;
    a.div = p->div;
    a.oslope = p->oslope;
    a.oslope2 = p->oslope2;
    a.wn_split = p->wn_split;
    a.out_pl = p->pl_rows ? dpl : nullptr;
    a.pl_rows = p->pl_rows;
    const bool name_was_on = g_launch_name_on;
    g_launch_name_on = true;
    g_launch_name[0] = 0;
    const hipError_t le = launch_conv(a, d.cfg, B, nullptr);
    g_launch_name_on = name_was_on;
    TCHECK(le);
    std::snprintf(p->kernel, sizeof p->kernel, "%s", g_launch_name);
    p->cfg_used = d.cfg;
    p->ck_used = d.CK;
    if (p->pl_rows) sx_unblock_kernel<<<dim3((T + 255) / 256, p->pl_rows / 8, B), 256>>>(nullptr, dpl, dpo, p->pl_rows, T, 1);
    TCHECK(hipGetLastError());
    TCHECK(hipDeviceSynchronize());
    TCHECK(download(p->out, dout, no));
    if (p->out2) TCHECK(download(p->out2, dout2, no));
    if (p->pl_rows) TCHECK(download(p->planes_out, dpo, (size_t)B * p->pl_rows * T));
    return VITS_OK;
}

int vits_test_wn_gate(int device_id, const float *a, int B, int H, int T, int form, float *acts) {
    if (int rc = test_dev(device_id)) return rc;
    if (!a || !acts || B < 1 || H < 1 || T < 1 || (form != 0 && form != 1)) return fail(nullptr, VITS_E_ARG, "bad gate test arguments");
    if (form == 1 && H % 8) return fail(nullptr, VITS_E_ARG, "the blocked gate reads cells of 8 channels: H %% 8 == 0");
    const size_t na = (size_t)B * 2 * H * T, no = (size_t)B * H * T;
    DevBufs D;
    float *da = D.up(a, na, 16);
    float *draw = D.alloc<float>(na, 16);
    float *dacts = D.fill<float>(no, 0xff, 16);
    TCHECK(D.err);
    if (form == 1) {
        sx_block_kernel<<<dim3((T + 255) / 256, 2 * H / 8, B), 256>>>(da, (int64_t)2 * H * T, T, nullptr, draw, 2 * H, T);
        wn_gate_blocked_kernel<<<dim3((T + 255) / 256, H / 8, B), 256>>>(draw, dacts, H, T);
    } else
        wn_gate_kernel<<<dim3((T + 255) / 256, H, B), 256>>>(da, dacts, H, T);
    TCHECK(hipGetLastError());
    TCHECK(hipDeviceSynchronize());
    TCHECK(download(acts, dacts, no));
    return VITS_OK;
}

int vits_test_cond_matvec(int device_id, const float *emb_g, int n_speakers, int gin, const int64_t *sid, int B, const float *W,
                          const float *bias, int rows, float *out) {
    if (int rc = test_dev(device_id)) return rc;
    if (!emb_g || !sid || !W || !out || n_speakers < 1 || gin < 1 || B < 1 || rows < 1)
        return fail(nullptr, VITS_E_ARG, "bad conditioning test arguments");
    DevBufs D;
    float *dg = D.up(emb_g, (size_t)n_speakers * gin);
    int64_t *dsid = D.up(sid, (size_t)B);
    float *dW = D.up(W, (size_t)rows * gin);
    float *db = bias ? D.up(bias, (size_t)rows) : nullptr;
    float *dout = D.fill<float>((size_t)B * rows, 0xff);
    TCHECK(D.err);
    cond_matvec_kernel<<<dim3((rows + 63) / 64, B), 64>>>(dg, dsid, n_speakers, dW, db, dout, rows, gin);
    TCHECK(hipGetLastError());
    TCHECK(hipDeviceSynchronize());
    TCHECK(download(out, dout, (size_t)B * rows));
    return VITS_OK;
}

// the test hooks' format of a split-operand conv: two fp16 planes unless stated otherwise
static TestPack sx_test_pack(SxPack::Planes planes = SxPack::F16X2) {
    TestPack o;
    o.sx.planes = planes;
    return o;
}

// ---- the same hooks through the split-operand engine: planar host tensors are converted to the engine's
// plane / raw layouts on the device, the result is converted back.
static int run_test_conv_sx(const ConvDesc &d, const std::vector<float> &arena, const float *x, int B, int T, int flags,
                            float slope, float *out) {
    const int Cr = d.Cout / d.ups, To = T * d.ups;
    const size_t nx = (size_t)B * d.Cin * T, no = (size_t)B * Cr * To;
    if ((flags & 4) && (d.Cin != d.Cout || d.ups != 1)) return fail(nullptr, VITS_E_ARG, "residual test needs Cin == Cout");
    std::vector<float> xa;
    if (d.h1 && (flags & 8)) {
        // single-plane mode with an input slope: the plane holds leaky_relu(x, slope) - what the conv consumes - and the
        // residual x is recovered from it (out = conv(lrelu(x)) + x): activate on the host, then store
        xa.resize(nx);
        for (size_t i = 0; i < nx; i++) xa[i] = x[i] >= 0.f ? x[i] : x[i] * slope;
        x = xa.data();
    }
    DevBufs D;
    float *dA = D.up(arena.data(), arena.size());
    float *dx = D.up(x, nx, 16);
    uint16_t *dxp = D.alloc<uint16_t>(nx * 3, 16);
    float *draw = D.fill<float>(no, 0, 16);
    uint16_t *dop = D.fill<uint16_t>(no * 3, 0, 16);
    float *dout = D.alloc<float>(no, 16);
    float *dres = D.alloc<float>(nx, 16);  // x in the raw layout: raw-input operand and residual
    TCHECK(D.err);
    sx_split_planes_kernel<<<dim3((T + 255) / 256, d.Cin / 8, B), 256>>>(dx, (int64_t)d.Cin * T, T, nullptr, dxp, d.Cin, T,
                                                                         d.h1 ? 2 : (d.f16 ? 1 : 0));
    sx_block_kernel<<<dim3((T + 255) / 256, d.Cin / 8, B), 256>>>(dx, (int64_t)d.Cin * T, T, nullptr, dres, d.Cin, T);
    SxArgs a = sx_args(d, dA, dA, T);  // (pack_test_* reserve a zero page at offset 0)
    a.xp = reinterpret_cast<const u32x4 *>(dxp);
    a.xr = dres;
    a.islope = (flags & 8) ? slope : 1.f;  // (raw-input convs only)
    a.out_raw = (flags & 128) ? nullptr : draw;  // (bit 7: planes are the only output - the specialised plane epilogues)
    a.out_pl = dop;
    a.oslope = 1.f;
    a.oslope2 = (flags & 1) ? slope : 1.f;
    if (flags & 4) {  // residual: res = x (same shape only)
        if (d.h1) {
            a.res_pl = dxp;  // the residual is the input plane itself, un-activated on the way in
            a.res_unslope = (flags & 8) ? 1.f / slope : 1.f;
        } else
            a.res = dres;
        a.flags |= EPI_RES;
    }
    const int nprod = d.h1 ? 1 : (d.f16 ? 2 : 6);
    if (flags & 256) {  // the short-launch kernel (conv_sx_small.hip.hpp) with the generator's epilogue
        if (!conv_sx_small_ok(a, d.rawin, nprod)) return fail(nullptr, VITS_E_ARG, "arguments not taken by the short-launch kernel");
        TCHECK(launch_conv_sx_small(a, B, d.cfg, nullptr));
    } else
        TCHECK(launch_conv_sx(a, d.cfg, B, nullptr, d.rawin, nprod));
    sx_unblock_kernel<<<dim3((To + 255) / 256, Cr / 8, B), 256>>>(draw, (flags & 1) ? dop : nullptr, dout, Cr, To,
                                                                  d.h1 ? 2 : (d.f16 ? 1 : 0));
    TCHECK(hipGetLastError());
    TCHECK(hipDeviceSynchronize());
    TCHECK(download(out, dout, no));
    return VITS_OK;
}

int vits_test_conv1d_sx(int device_id, const float *x, int B, int Cin, int T, const float *w, const float *bias, int Cout,
                        int K, int dil, int pad_l, int flags, float slope, float *out) {
    if (int rc = test_dev(device_id)) return rc;
    ConvDesc d;
    std::vector<float> arena;
    const int prec = (flags >> 4) & 3;  // 0: bf16x6, 3: f16x3 (two fp16 planes), 2: f16 (one fp16 plane, one product)
    if (prec == 1) return fail(nullptr, VITS_E_ARG, "precision code 1 (bf16x3) was retired");
    if ((flags & 128) && !(flags & 1)) return fail(nullptr, VITS_E_ARG, "planes-only output is read back from the planes (bit 0)");
    const TestPack o = sx_test_pack(prec == 2 ? SxPack::F16X1 : (prec == 3 ? SxPack::F16X2 : SxPack::BF16X3));
    std::string e = pack_test_conv(w, bias, Cin, Cout, K, dil, pad_l, 3, &d, &arena, o);
    if (!e.empty()) return fail(nullptr, VITS_E_ARG, "%s", e.c_str());
    return run_test_conv_sx(d, arena, x, B, T, flags, slope, out);
}

// The split-operand engine with conv_sx()'s whole argument set (include/vitsmi.h): sx_args() plus the field assignments
// conv_sx() makes, one launch_conv_sx() on the run tile asked for.  What launch_conv_sx() would refuse is refused here by
// name; both outputs start as the sentinel (or the old contents), so what the launch did not write reads back unchanged.
int vits_test_conv1d_sx_epi(int device_id, vits_test_conv_sx_epi_args *p) {
    if (int rc = test_dev(device_id)) return rc;
    if (!p) return fail(nullptr, VITS_E_ARG, "no arguments");
    const auto bad = [](const char *why) { return fail(nullptr, VITS_E_ARG, "sx conv epilogue hook: %s", why); };
    const int B = p->B, Cin = p->Cin, T = p->T, Cr = p->Cout, u = p->stride, flags = p->flags;
    if (B < 1 || Cin < 1 || T < 1 || Cr < 1 || u < 1 || !p->x || !p->w) return bad("bad shape or missing tensor");
    if (flags & ~(VITS_SX_EPI_RES | VITS_SX_EPI_ACC | VITS_SX_EPI_DIV | VITS_SX_EPI_NO_RAW_STORE)) return bad("unknown flag");
    if (p->precision < VITS_SX_BF16X6 || p->precision > VITS_SX_F16) return bad("precision: bf16x6, f16x3 or f16");
    if (Cin % 16 || Cr % 32) return bad("Cin % 16 == 0 and Cout % 32 == 0");
    if (p->run_cfg < -1 || p->run_cfg > 3 || p->min_cfg < 0 || p->min_cfg > 3) return bad("tile configs are 0..3");
    if (u == 1 && (p->K < 1 || p->dil < 1 || p->pad_l < 0 || p->pad_l > (int64_t)p->dil * (p->K - 1))) return bad("pad_l outside the receptive field");
    const bool want_raw = p->out != nullptr, want_pl = p->planes_out != nullptr;
    const bool f_res = flags & VITS_SX_EPI_RES, f_acc = flags & VITS_SX_EPI_ACC;
    if (!want_raw && !want_pl) return bad("neither a raw nor a plane output");
    if (f_acc && !want_raw) return bad("acc without a raw tensor (the accumulate operand is out's previous contents)");
    if ((flags & VITS_SX_EPI_NO_RAW_STORE) && !want_raw) return bad("no_raw_store without a raw tensor");
    if (p->old_out && !want_raw) return bad("old_out without a raw tensor");
    const int res_forms = (p->res ? 1 : 0) + (p->res_is_x ? 1 : 0);
    if (f_res && res_forms != 1) return bad("res needs exactly one form: a tensor (fp32, or as planes with res_planes) or res_is_x");
    if (!f_res && (res_forms || p->res_planes)) return bad("a residual operand without the res flag");
    if (p->res_planes && (!p->res || !(p->res_slope > 0.f))) return bad("res_planes needs the res tensor and res_slope > 0");
    if (p->bias_b && p->bias_b_stride < Cr) return bad("bias_b rows shorter than Cout");
    if (p->rag_mul < 1 && p->lens) return bad("rag_mul < 1");
    if (p->lens)
        for (int b = 0; b < B; b++)
            if (p->lens[b] < 0 || p->lens[b] > T) return bad("lens outside [0, T]");
    ConvDesc d;
    std::vector<float> arena;
    TestPack o;
    o.sx.planes = p->precision == VITS_SX_F16 ? SxPack::F16X1 : (p->precision == VITS_SX_F16X3 ? SxPack::F16X2 : SxPack::BF16X3);
    o.sx.force16 = p->force16 != 0;
    o.sx.no_s16 = p->no_s16 != 0;
    o.sx.min_cfg = p->min_cfg;
    {
        const std::string e = u > 1 ? pack_test_convT(p->w, p->bias, Cin, Cr, p->K, u, &d, &arena, true, o)
                                    : pack_test_conv(p->w, p->bias, Cin, Cr, p->K, p->dil, p->pad_l, 3, &d, &arena, o);
        if (!e.empty()) return fail(nullptr, VITS_E_ARG, "%s", e.c_str());
    }
    // ---- launch_conv_sx()'s refusals, by name
    const int nprod = d.h1 ? 1 : (d.f16 ? 2 : 6), run = p->run_cfg >= 0 ? p->run_cfg : d.cfg;
    if (d.rawin && run == 0) return bad("raw input on cfg 0: the raw-input kernels exist for the 64- and 32-row tiles only");
    if (run == 3 && !d.s16) return bad("run_cfg 3 without s16: the 64 x 128 tile exists on the 16x16x32 loop only");
    if (sx_tile_m(run) > sx_tile_m(d.cfg)) return bad("a run tile taller than the packed one");
    if (!sx_tile_reads(d.cfg, run, d.s16) || d.Cout % sx_tile_m(run)) return bad("the run tile cannot read this packing");
    if (d.rawin && run != d.cfg) return bad("a raw-input conv runs on the tile it was packed for");
    if (!sx_stage(sx_tile_n(run), d.K, d.dil, nprod == 6 ? 3 : nprod, d.s16).fits) return bad("the x stage does not fit the run tile");
    if (p->islope != 0.f && p->islope != 1.f && !d.rawin) return bad("islope on a plane-input conv (the raw-input prologue applies it)");
    if (p->res_is_x && (!d.rawin || Cin != Cr || u != 1)) return bad("res_is_x needs a raw-input conv with Cin == Cout");
    if (p->res_planes && d.rawin) return bad("res_planes on raw input: a raw-input conv reads its residual as fp32");
    if (p->res_planes && nprod == 6) return bad("res_planes in bf16x6: only the fp16 arithmetics read a residual from planes");
    if (f_res && nprod == 1 && !p->res_planes) return bad("the single-plane arithmetic reads its residual from a plane (res_planes)");
    const int To = T * u, mode = d.h1 ? 2 : (d.f16 ? 1 : 0);
    const size_t nx = (size_t)B * Cin * T, no = (size_t)B * Cr * To;
    // host images: the raw output (old contents, else the sentinel), the sentinel whose planes pre-fill the plane output,
    // the residual as its planes hold it
    std::vector<float> ho(no, p->sentinel), hs(no, p->sentinel), hr;
    if (p->old_out) std::memcpy(ho.data(), p->old_out, no * 4);
    if (p->res_planes) {
        hr.resize(no);
        for (size_t i = 0; i < no; i++) hr[i] = p->res[i] >= 0.f ? p->res[i] : p->res[i] * p->res_slope;
    }
    std::vector<int> l32(B);
    for (int b = 0; b < B; b++) l32[b] = p->lens ? (int)p->lens[b] : T;
    DevBufs D;
    float *dA = D.up(arena.data(), arena.size());
    float *dx = D.up(p->x, nx, 16);
    uint16_t *dxp = d.rawin ? nullptr : D.fill<uint16_t>(nx * 3, 0, 64);
    float *dxr = d.rawin ? D.alloc<float>(nx, 64) : nullptr;
    float *dimg = want_raw ? D.up(ho.data(), no, 16) : nullptr;
    float *draw = want_raw ? D.alloc<float>(no, 64) : nullptr;
    float *dsen = want_pl ? D.up(hs.data(), no, 16) : nullptr;
    uint16_t *dop = want_pl ? D.fill<uint16_t>(no * 3, 0, 64) : nullptr;
    float *dout = D.alloc<float>(no, 16);
    float *dresin = p->res ? D.up(p->res_planes ? hr.data() : p->res, no, 16) : nullptr;
    float *dres = (p->res && !p->res_planes) ? D.alloc<float>(no, 64) : nullptr;
    uint16_t *dresp = p->res_planes ? D.fill<uint16_t>(no * 3, 0, 64) : nullptr;
    float *dbb = p->bias_b ? D.up(p->bias_b, (size_t)B * p->bias_b_stride) : nullptr;
    int *dlen = p->lens ? D.up(l32.data(), (size_t)B) : nullptr;
    unsigned *dpk = mode ? D.fill<unsigned>((size_t)kSxPeakSlots * kSxPeakStride) : nullptr;
    TCHECK(D.err);
    const dim3 gin((T + 255) / 256, Cin / 8, B), gout((To + 255) / 256, Cr / 8, B);
    if (d.rawin) sx_block_kernel<<<gin, 256>>>(dx, (int64_t)Cin * T, T, nullptr, dxr, Cin, T);
    else sx_split_planes_kernel<<<gin, 256>>>(dx, (int64_t)Cin * T, T, nullptr, dxp, Cin, T, mode);
    if (want_raw) sx_block_kernel<<<gout, 256>>>(dimg, (int64_t)Cr * To, To, nullptr, draw, Cr, To);
    if (want_pl) sx_split_planes_kernel<<<gout, 256>>>(dsen, (int64_t)Cr * To, To, nullptr, dop, Cr, To, mode);
    if (dres) sx_block_kernel<<<gout, 256>>>(dresin, (int64_t)Cr * To, To, nullptr, dres, Cr, To);
    if (dresp) sx_split_planes_kernel<<<gout, 256>>>(dresin, (int64_t)Cr * To, To, nullptr, dresp, Cr, To, mode);
    TCHECK(hipGetLastError());
    SxArgs a = sx_args(d, dA, dA, T);  // (pack_test_* reserve a zero page at offset 0)
    a.xp = reinterpret_cast<const u32x4 *>(dxp);
    a.xr = dxr;
    a.islope = p->islope;
    a.bias_b = dbb;
    a.bias_b_stride = p->bias_b_stride;
    a.out_raw = draw;
    a.out_pl = dop;
    a.res = p->res_is_x ? dxr : dres;
    a.res_pl = dresp;
    a.res_unslope = p->res_planes ? 1.f / p->res_slope : 1.f;
    a.flags = (f_res ? EPI_RES : 0) | (f_acc ? EPI_ACC : 0) | ((flags & VITS_SX_EPI_DIV) ? EPI_DIV : 0) |
              ((flags & VITS_SX_EPI_NO_RAW_STORE) ? SX_NO_RAW_STORE : 0);
    a.div = p->div == 0.f ? 1.f : p->div;
    a.oslope = p->oslope;
    a.oslope2 = p->oslope2;
    a.rag = SxRagged{dlen, p->rag_add, p->rag_mul};
    a.peak = dpk;
    const bool name_was_on = g_launch_name_on;
    g_launch_name_on = true;
    g_launch_name[0] = 0;
    const hipError_t le = launch_conv_sx(a, run, B, nullptr, d.rawin, nprod, d.cfg);
    g_launch_name_on = name_was_on;
    if (le != hipSuccess) return fail(nullptr, VITS_E_DEVICE, "sx conv epilogue hook: launch_conv_sx: %s", hipGetErrorString(le));
    std::snprintf(p->kernel, sizeof p->kernel, "%s", g_launch_name);
    p->pack_cfg = d.cfg;
    p->run_cfg_used = run;
    p->rawin = d.rawin ? 1 : 0;
    p->s16 = d.s16 ? 1 : 0;
    p->ck = d.CK;
    p->peak = 0.f;
    if (want_raw) {
        sx_unblock_kernel<<<gout, 256>>>(draw, nullptr, dout, Cr, To, mode);
        TCHECK(hipGetLastError());
        TCHECK(hipDeviceSynchronize());
        TCHECK(download(p->out, dout, no));
    }
    if (want_pl) {
        sx_unblock_kernel<<<gout, 256>>>(nullptr, dop, dout, Cr, To, mode);
        TCHECK(hipGetLastError());
        TCHECK(hipDeviceSynchronize());
        TCHECK(download(p->planes_out, dout, no));
    }
    if (dresp && p->res_seen) {
        sx_unblock_kernel<<<gout, 256>>>(nullptr, dresp, dout, Cr, To, mode);
        TCHECK(hipGetLastError());
        TCHECK(hipDeviceSynchronize());
        TCHECK(download(p->res_seen, dout, no));
    }
    TCHECK(hipDeviceSynchronize());
    if (dpk) {
        std::vector<unsigned> slots((size_t)kSxPeakSlots * kSxPeakStride);
        TCHECK(download(slots.data(), dpk, slots.size()));
        unsigned top = 0;
        for (int s = 0; s < kSxPeakSlots; s++) top = std::max(top, slots[(size_t)s * kSxPeakStride]);
        std::memcpy(&p->peak, &top, 4);
    }
    return VITS_OK;
}

int vits_test_conv1d_sx_planar(int device_id, const float *x, int B, int Cin, int T, const float *w, const float *bias,
                               int Cout, int K, int dil, int flags, const int64_t *lens, const float *old, int row_split,
                               int pl_rows, float *out, float *planes_out) {
    // the planar epilogue of the split-operand engine (f16x3, 16x16x32 loop), as the flow and the text encoder use it:
    // flags bit 0 ReLU, 1 mask (t < lens[b]), 2 residual (old: planar [B][row_split][T]), 3 accumulate (old: the
    // outputs' previous contents, [B][Cout][T]), 4 coupling update, 5 the rows behind row_split are stored (not
    // accumulated), 6 the planes are those of the rows behind row_split, 7 run the short-launch kernel.  out = [B][Cout][T] (rows behind row_split from
    // the second tensor); planes_out (nullable) = [B][pl_rows][T] read back from the operand planes.
    if (int rc = test_dev(device_id)) return rc;
    if (Cin % 32 || Cout % 32 || row_split % 32 || row_split > Cout || pl_rows % 32) return fail(nullptr, VITS_E_ARG, "bad planar test shape");
    ConvDesc d;
    std::vector<float> arena;
    std::string e = pack_test_conv(w, bias, Cin, Cout, K, dil, dil * (K - 1) / 2, 3, &d, &arena, sx_test_pack());
    if (!e.empty()) return fail(nullptr, VITS_E_ARG, "%s", e.c_str());
    if (!d.s16) return fail(nullptr, VITS_E_ARG, "shape not taken by the 16x16x32 loop");
    const int srows = Cout - row_split;
    const size_t nx = (size_t)B * Cin * T, n1 = (size_t)B * (row_split ? row_split : 1) * T, n2 = (size_t)B * (srows ? srows : 1) * T;
    const size_t npl = (size_t)B * (pl_rows ? pl_rows : 32) * T;
    std::vector<int> l32(B);
    for (int b = 0; b < B; b++) l32[b] = lens ? (int)lens[b] : T;
    DevBufs D;
    float *dA = D.up(arena.data(), arena.size());
    float *dx = D.up(x, nx, 16);
    uint16_t *dxp = D.alloc<uint16_t>(nx * 3, 64);
    float *d1 = D.fill<float>(n1, 0, 16);
    float *d2 = D.fill<float>(n2, 0, 16);
    float *dres = D.fill<float>(n1, 0, 16);
    uint16_t *dpl = D.alloc<uint16_t>(npl * 3, 64);
    float *dpo = D.alloc<float>(npl, 16);
    int *dlen = D.up(l32.data(), (size_t)B);
    TCHECK(D.err);
    if (old) {
        // [B][Cout][T] -> the two planar tensors (accumulate / coupling) or the residual (rows of the first tensor)
        for (int b = 0; b < B; b++) {
            if (row_split)
                TCHECK(hipMemcpy(((flags & 4) ? dres : d1) + (size_t)b * row_split * T, old + (size_t)b * Cout * T, (size_t)row_split * T * 4,
                                 hipMemcpyHostToDevice));
            if (srows && !(flags & 4))
                TCHECK(hipMemcpy(d2 + (size_t)b * srows * T, old + ((size_t)b * Cout + row_split) * T, (size_t)srows * T * 4,
                                 hipMemcpyHostToDevice));
        }
    }
    sx_split_planes_kernel<<<dim3((T + 255) / 256, Cin / 8, B), 256>>>(dx, (int64_t)Cin * T, T, nullptr, dxp, Cin, T, 1);
    SxArgs a = sx_args(d, dA, dA, T);  // (pack_test_* reserve a zero page at offset 0)
    a.xp = reinterpret_cast<const u32x4 *>(dxp);
    a.out_raw = row_split ? d1 : nullptr;
    a.out_raw2 = srows ? d2 : nullptr;
    a.row_split = row_split;
    a.len = dlen;
    a.res = (flags & 4) ? dres : nullptr;
    a.out_pl = pl_rows ? dpl : nullptr;
    a.pl_rows = pl_rows;
    a.pl_of2 = (flags & 64) ? 1 : 0;
    a.pl_bstride = (int64_t)3 * pl_rows * T;
    a.flags = SX_WN_RMW | ((flags & 1) ? EPI_RELU : 0) | ((flags & 2) ? EPI_MASK : 0) | ((flags & 4) ? EPI_RES : 0) |
              ((flags & 8) ? EPI_ACC : 0) | ((flags & 16) ? SX_PLANAR_COUPLING : 0) | ((flags & 32) ? SX_PLANAR_STORE2 : 0);
    if (flags & 128) {  // the short-launch kernel (conv_sx_small.hip.hpp) instead of the engine's
        if (!conv_sx_small_ok(a, false, 2)) return fail(nullptr, VITS_E_ARG, "arguments not taken by the short-launch kernel");
        TCHECK(launch_conv_sx_small(a, B, d.cfg, nullptr));
    } else
        TCHECK(launch_conv_sx(a, d.cfg, B, nullptr, false, 2));
    if (pl_rows)
        sx_unblock_kernel<<<dim3((T + 255) / 256, pl_rows / 8, B), 256>>>(nullptr, dpl, dpo, pl_rows, T, 1);
    TCHECK(hipGetLastError());
    TCHECK(hipDeviceSynchronize());
    for (int b = 0; b < B; b++) {
        if (row_split) TCHECK(download(out + (size_t)b * Cout * T, d1 + (size_t)b * row_split * T, (size_t)row_split * T));
        if (srows) TCHECK(download(out + ((size_t)b * Cout + row_split) * T, d2 + (size_t)b * srows * T, (size_t)srows * T));
    }
    if (pl_rows && planes_out) TCHECK(download(planes_out, dpo, (size_t)B * pl_rows * T));
    return VITS_OK;
}

// A/B hook: the short-launch kernel's launch-size limit (0 = every launch on the engine); returns the previous value
long long vits_test_set_sx_small_max(long long wgs) { return sx_small_max().exchange(wgs); }

// The WN in-layer with its gate epilogue (SX_GATE; f16x3, 16x16x32 loop): acts = tanh(a + g_a) * sigmoid(b + g_b), a / b = the
// conv's rows.  w / bias arrive in the PACKED row order (32 tanh rows, their 32 sigmoid partners, the next 32 tanh rows, ..: what
// model.cpp's out_perm produces), bias_b [B][Cout] (the per-utterance conditioning) in the module's order (tanh half, sigmoid
// half).  flags bit 0: the short-launch kernel (conv_sx_small.hip.hpp) instead of the engine's; bit 1: acts through the fp16
// operand planes instead of the planar fp32 output.  out = [B][Cout / 2][T].
int vits_test_conv1d_sx_gate(int device_id, const float *x, int B, int Cin, int T, const float *w, const float *bias,
                             const float *bias_b, int Cout, int K, int dil, int flags, float *out) {
    if (int rc = test_dev(device_id)) return rc;
    if (Cin % 32 || Cout % 64) return fail(nullptr, VITS_E_ARG, "bad gate test shape");
    ConvDesc d;
    std::vector<float> arena;
    std::string e = pack_test_conv(w, bias, Cin, Cout, K, dil, dil * (K - 1) / 2, 3, &d, &arena, sx_test_pack());
    if (!e.empty()) return fail(nullptr, VITS_E_ARG, "%s", e.c_str());
    if (!d.s16) return fail(nullptr, VITS_E_ARG, "shape not taken by the 16x16x32 loop");
    const int H = Cout / 2;
    const size_t nx = (size_t)B * Cin * T, no = (size_t)B * H * T;
    DevBufs D;
    float *dA = D.up(arena.data(), arena.size());
    float *dx = D.up(x, nx, 16);
    uint16_t *dxp = D.alloc<uint16_t>(nx * 3, 64);
    float *dact = D.fill<float>(no, 0xff, 16);
    uint16_t *dpl = D.alloc<uint16_t>(no * 3, 64);
    float *dbb = D.up(bias_b, (size_t)B * Cout);
    TCHECK(D.err);
    sx_split_planes_kernel<<<dim3((T + 255) / 256, Cin / 8, B), 256>>>(dx, (int64_t)Cin * T, T, nullptr, dxp, Cin, T, 1);
    SxArgs a = sx_args(d, dA, dA, T);  // (pack_test_* reserve a zero page at offset 0)
    a.xp = reinterpret_cast<const u32x4 *>(dxp);
    a.bias_b = dbb;
    a.bias_b_stride = Cout;
    a.flags = SX_GATE;
    a.raw_bstride = (int64_t)H * T;
    a.pl_bstride = (int64_t)3 * H * T;
    if (flags & 2) a.out_pl = dpl;
    else a.out_raw = dact;
    if (flags & 1) {
        if (!conv_sx_small_ok(a, false, 2)) return fail(nullptr, VITS_E_ARG, "arguments not taken by the short-launch kernel");
        TCHECK(launch_conv_sx_small(a, B, d.cfg, nullptr));
    } else
        TCHECK(launch_conv_sx(a, d.cfg == 0 ? 3 : d.cfg, B, nullptr, false, 2, d.cfg));
    if (flags & 2) sx_unblock_kernel<<<dim3((T + 255) / 256, H / 8, B), 256>>>(nullptr, dpl, dact, H, T, 1);
    TCHECK(hipGetLastError());
    TCHECK(hipDeviceSynchronize());
    TCHECK(download(out, dact, no));
    return VITS_OK;
}

int vits_test_conv_transpose1d_sx(int device_id, const float *x, int B, int Cin, int T, const float *w, const float *bias,
                                  int Cout, int K, int stride, float *out) {
    if (int rc = test_dev(device_id)) return rc;
    ConvDesc d;
    std::vector<float> arena;
    const bool f16 = stride < 0;  // (test hook convention: negative stride = the fp16 two-plane mode)
    if (f16) stride = -stride;
    std::string e = pack_test_convT(w, bias, Cin, Cout, K, stride, &d, &arena, true, sx_test_pack(f16 ? SxPack::F16X2 : SxPack::BF16X3));
    if (!e.empty()) return fail(nullptr, VITS_E_ARG, "%s", e.c_str());
    return run_test_conv_sx(d, arena, x, B, T, 0, 0.f, out);
}

// The fused ResBlock step as conv_sx_pair16() launches it (include/vitsmi.h): SxPair16Args from sx_pair16_args(), the
// generator's own filler, one launch_conv_sx_pair16().  The raw tensor starts as old_out or the sentinel, the planes as the
// sentinel's split, both with a guard band of one 256-column tile row of sentinel cells behind the last utterance: what the
// launch did not write reads back unchanged.
int vits_test_conv_pair16_epi(int device_id, vits_test_conv_pair16_epi_args *p) {
    if (int rc = test_dev(device_id)) return rc;
    if (!p) return fail(nullptr, VITS_E_ARG, "no arguments");
    const auto bad = [](const char *why) { return fail(nullptr, VITS_E_ARG, "pair16 epilogue hook: %s", why); };
    const int B = p->B, C = p->C, T = p->T, K = p->K, flags = p->flags;
    if (B < 1 || C < 1 || T < 1 || K < 1 || p->dil1 < 1 || p->dil2 < 1 || !p->x || !p->w1 || !p->w2) return bad("bad shape or missing tensor");
    if (flags & ~(VITS_P16_EPI_ACC | VITS_P16_EPI_DIV | VITS_P16_EPI_RAW | VITS_P16_EPI_PLANES)) return bad("unknown flag");
    if (p->precision != VITS_SX_F16X3 && p->precision != VITS_SX_F16) return bad("precision: f16x3 or f16");
    if (C % 32) return bad("C % 32 == 0");
    if (!(p->slope > 0.f)) return bad("slope > 0 (the residual is recovered by undoing it)");
    if ((flags & VITS_P16_EPI_ACC) && !p->old_out) return bad("acc without old_out (the accumulate operand is the raw tensor's previous contents)");
    if (p->lens && p->rag_mul < 1) return bad("rag_mul < 1");
    if (p->lens)
        for (int b = 0; b < B; b++)
            if (p->lens[b] < 0 || p->lens[b] > T) return bad("lens outside [0, T]");
    const bool h1 = p->precision == VITS_SX_F16, chain = p->chain != 0;
    const int npl = h1 ? 1 : 2, mode = h1 ? 2 : 1;
    ConvDesc d1, d2;
    std::vector<float> arena;
    TestPack o = sx_test_pack(h1 ? SxPack::F16X1 : SxPack::F16X2);
    o.sx.force16 = !h1;  // (the pair16 kernel takes its 32- / 64-channel weights in the 16x16x32 layout)
    std::string e = pack_test_conv(p->w1, p->b1, C, C, K, p->dil1, p->dil1 * (K - 1) / 2, 3, &d1, &arena, o);
    if (e.empty()) e = pack_test_conv(p->w2, p->b2, C, C, K, p->dil2, p->dil2 * (K - 1) / 2, 3, &d2, &arena, o);
    if (!e.empty()) return fail(nullptr, VITS_E_ARG, "%s", e.c_str());
    if (!d1.s16 || !d2.s16 || d1.rawin || d2.rawin || !sx_pair16_plan(C, npl, d1.K, d1.dil, d2.K, d2.dil, nullptr))
        return fail(nullptr, VITS_E_ARG, "this conv pair cannot run fused on the 16x16x32 loop (C %d, kernel %d, dilations %d, %d)", C, K, p->dil1,
                    p->dil2);
    const size_t n = (size_t)B * C * T, CT = (size_t)C * T;
    const size_t G = 256 * 8;  // guard band behind each output: one tile row of cells
    const float slope = p->slope, sen = p->sentinel;
    // where each utterance's tensors end (sx_valid_cols)
    std::vector<int> l32(B), ends(B);
    for (int b = 0; b < B; b++) {
        l32[b] = p->lens ? (int)p->lens[b] : T;
        const long long v = l32[b] > 0 ? (long long)(l32[b] + p->rag_add) * p->rag_mul : 0;
        ends[b] = !p->lens ? T : (int)std::min<long long>(std::max<long long>(v, 0), T);
    }
    // host images: the input planes' content leaky_relu(x, slope) - x_tail behind each end -, the raw tensor, the sentinel
    std::vector<float> xa(n), ho(n, sen), hs(n, sen);
    for (int b = 0; b < B; b++)
        for (int c = 0; c < C; c++)
            for (int t = 0; t < T; t++) {
                const size_t i = ((size_t)b * C + c) * T + t;
                const float v = (p->x_tail && t >= ends[b]) ? p->x_tail[i] : p->x[i];
                xa[i] = v >= 0.f ? v : v * slope;
            }
    if (p->old_out) std::memcpy(ho.data(), p->old_out, n * 4);
    const _Float16 sen_h = (_Float16)std::min(std::max(sen, -kF16Max), kF16Max);
    const std::vector<float> graw(G, sen);
    const std::vector<uint16_t> gpl(G, __builtin_bit_cast(uint16_t, sen_h));
    DevBufs D;
    float *dA = D.up(arena.data(), arena.size());
    float *dx = D.up(xa.data(), n, 16);
    uint16_t *dxp = D.fill<uint16_t>(n * 3, 0, 64);
    float *dimg = D.up(ho.data(), n, 16);
    float *dsen = D.up(hs.data(), n, 16);
    float *draw = D.alloc<float>(n + G, 64);
    uint16_t *dop = D.fill<uint16_t>(n * 3 + G, 0, 64);
    float *dout = D.alloc<float>(n, 16);
    int *dlen = p->lens ? D.up(l32.data(), (size_t)B) : nullptr;
    unsigned *dpk = D.fill<unsigned>((size_t)kSxPeakSlots * kSxPeakStride);
    TCHECK(D.err);
    const dim3 grid((T + 255) / 256, C / 8, B);
    sx_split_planes_kernel<<<grid, 256>>>(dx, (int64_t)CT, T, nullptr, dxp, C, T, mode);
    sx_block_kernel<<<grid, 256>>>(dimg, (int64_t)CT, T, nullptr, draw, C, T);
    sx_split_planes_kernel<<<grid, 256>>>(dsen, (int64_t)CT, T, nullptr, dop, C, T, mode);
    TCHECK(hipGetLastError());
    TCHECK(hipMemcpy(draw + n, graw.data(), G * 4, hipMemcpyHostToDevice));
    TCHECK(hipMemcpy(dop + n * 3, gpl.data(), G * 2, hipMemcpyHostToDevice));
    const int kflags = ((flags & VITS_P16_EPI_ACC) ? EPI_ACC : 0) | ((flags & VITS_P16_EPI_DIV) ? EPI_DIV : 0) |
                       ((flags & VITS_P16_EPI_RAW) ? P16_HAS_RAW : 0) | ((flags & VITS_P16_EPI_PLANES) ? P16_HAS_PL : 0);
    const SxRagged rag = dlen ? SxRagged{dlen, p->rag_add, p->rag_mul} : SxRagged{nullptr, 0, 0};
    SxPair16Args a = sx_pair16_args(d1, d2, dA, dA, dxp, T, draw, dop, kflags, p->div == 0.f ? 1.f : p->div, slope, rag, dpk);  // (pack_test_* reserve a zero page at offset 0)
    SxPair16Tile tile{};
    auto go = [&] { return launch_conv_sx_pair16(a, C, npl, B, nullptr, chain, &tile); };
    const bool name_was_on = g_launch_name_on;
    g_launch_name_on = true;
    g_launch_name[0] = 0;
    const hipError_t le = go();
    g_launch_name_on = name_was_on;
    if (le != hipSuccess) return fail(nullptr, VITS_E_DEVICE, "pair16 epilogue hook: launch_conv_sx_pair16: %s", hipGetErrorString(le));
    TCHECK(hipDeviceSynchronize());
    std::snprintf(p->kernel, sizeof p->kernel, "%s", g_launch_name);
    p->BN = tile.BN;  // (the tile as the launcher reports it)
    p->BNo = tile.BNo;
    p->ovl = tile.ovl ? 1 : 0;
    if (p->out) {
        sx_unblock_kernel<<<grid, 256>>>(draw, nullptr, dout, C, T, mode);
        TCHECK(hipGetLastError());
        TCHECK(hipDeviceSynchronize());
        TCHECK(download(p->out, dout, n));
    }
    if (p->planes_out) {
        sx_unblock_kernel<<<grid, 256>>>(nullptr, dop, dout, C, T, mode);
        TCHECK(hipGetLastError());
        TCHECK(hipDeviceSynchronize());
        TCHECK(download(p->planes_out, dout, n));
    }
    if (p->x_seen) {
        sx_unblock_kernel<<<grid, 256>>>(nullptr, dxp, dout, C, T, mode);
        TCHECK(hipGetLastError());
        TCHECK(hipDeviceSynchronize());
        TCHECK(download(p->x_seen, dout, n));
        const float un = 1.f / slope;  // (read_x16: v < 0 ? v * un_islope : v)
        for (size_t i = 0; i < n; i++)
            if (p->x_seen[i] < 0.f) p->x_seen[i] *= un;
    }
    {
        std::vector<float> gr(G);
        std::vector<uint16_t> hp(n * 3 + G);
        TCHECK(download(gr.data(), draw + n, G));
        TCHECK(download(hp.data(), dop, hp.size()));
        bool ok = std::memcmp(gr.data(), graw.data(), G * 4) == 0 && std::memcmp(hp.data() + n * 3, gpl.data(), G * 2) == 0;
        for (int b = 0; b < B && ok; b++)  // the planes the arithmetic does not use
            for (size_t i = (size_t)npl * CT; i < 3 * CT && ok; i++) ok = hp[(size_t)b * 3 * CT + i] == 0;
        p->guard_ok = ok ? 1 : 0;
    }
    {
        std::vector<unsigned> slots((size_t)kSxPeakSlots * kSxPeakStride);
        TCHECK(download(slots.data(), dpk, slots.size()));
        unsigned top = 0;
        for (int s = 0; s < kSxPeakSlots; s++) top = std::max(top, slots[(size_t)s * kSxPeakStride]);
        std::memcpy(&p->peak, &top, 4);
    }
#if P16_PROF
    {
        const size_t nwg = 1 << 17;  // (>= the launch's workgroups)
        unsigned long long *dprof = D.fill<unsigned long long>(nwg * 8);
        TCHECK(D.err);
        a.prof = dprof;
        TCHECK(go());
        TCHECK(hipDeviceSynchronize());
        std::vector<unsigned long long> hp(nwg * 8);
        TCHECK(download(hp.data(), dprof, nwg * 8));
        // (a row per workgroup: phase sums over its tiles, [7] = tiles - one in the one-shot form, many in the persistent one)
        double sum[7] = {0, 0, 0, 0, 0, 0, 0};
        unsigned long long nt = 0, wgs = 0;
        for (size_t w = 0; w < nwg; w++)
            if (hp[w * 8 + 7]) {
                wgs++;
                nt += hp[w * 8 + 7];
                for (int i = 0; i < 7; i++) sum[i] += (double)hp[w * 8 + i];
            }
        fprintf(stderr, "p16prof C %d npl %d K %d wgs %llu tiles %llu | x wait %.0f  barrier %.0f  phase1 %.0f  hand-over %.0f  phase2 %.0f  epilogue %.0f  drain %.0f (cycles per TILE)\n",
                C, npl, K, wgs, nt, sum[0] / nt, sum[1] / nt, sum[2] / nt, sum[3] / nt, sum[4] / nt, sum[5] / nt, sum[6] / nt);
        a.prof = nullptr;
    }
#endif
    // (behind the read-back: with ACC every further launch accumulates again)
    if (p->ms_out) TCHECK(time_launches(10, go, p->ms_out));
    return VITS_OK;
}

// Two dependent convs through ONE fused launch (include/vitsmi.h): chain bit 0 = CHAIN (two ResBlock2 steps, else a ResBlock1
// step), bits 1-2 = kernel: 0 conv_sx_pair_kernel (conv_sx_pair.hip.hpp: 32x32x16 form, f16x3, fp32 raw tensors), 1
// conv_sx_pair16_kernel in f16x3, 2 the same in the single-plane arithmetic (both: operand planes of leaky_relu(x) in); bit 3
// (pair16 only): the result is read back from the output PLANES (leaky_relu(out, slope)) instead of the fp32 output.
// x, out: [B, C, T] host; w1, w2: [C, C, K]; c1 dilated by dil1, c2 by dil2; ms_out (nullable): the launch is also timed.
int vits_test_conv_pair_sx(int device_id, const float *x, int B, int C, int T, const float *w1, const float *b1,
                           const float *w2, const float *b2, int K, int dil1, int dil2, int chain, float slope, float *out,
                           float *ms_out) {
    if (int rc = test_dev(device_id)) return rc;
    const int kern = (chain >> 1) & 3;
    const bool from_plane = (chain & 8) != 0;
    chain &= 1;
    if (kern) {  // the pair16 forms: vits_test_conv_pair16_epi's launch with `raw` or `planes`, no lens, zero-filled buffers
        vits_test_conv_pair16_epi_args e{};
        e.B = B, e.C = C, e.T = T, e.K = K, e.dil1 = dil1, e.dil2 = dil2, e.chain = chain;
        e.precision = kern == 2 ? VITS_SX_F16 : VITS_SX_F16X3;
        e.flags = from_plane ? VITS_P16_EPI_PLANES : VITS_P16_EPI_RAW;
        e.slope = slope, e.div = 1.f, e.sentinel = 0.f;
        e.x = x, e.w1 = w1, e.b1 = b1, e.w2 = w2, e.b2 = b2;
        (from_plane ? e.planes_out : e.out) = out;
        e.ms_out = ms_out;
        return vits_test_conv_pair16_epi(device_id, &e);
    }
    ConvDesc d1, d2;
    std::vector<float> arena;
    const TestPack o = sx_test_pack(SxPack::F16X2);
    std::string e = pack_test_conv(w1, b1, C, C, K, dil1, dil1 * (K - 1) / 2, 3, &d1, &arena, o);
    if (e.empty()) e = pack_test_conv(w2, b2, C, C, K, dil2, dil2 * (K - 1) / 2, 3, &d2, &arena, o);
    if (!e.empty()) return fail(nullptr, VITS_E_ARG, "%s", e.c_str());
    const size_t n = (size_t)B * C * T;
    DevBufs D;
    if (!d1.rawin || !d2.rawin || d1.cfg != d2.cfg || !sx_pair_supported(C, d1.cfg, d1.K, d1.dil, d2.K, d2.dil))
        return fail(nullptr, VITS_E_ARG, "this conv pair cannot run fused (C %d, kernel %d, dilation %d)", C, K, dil1);
    float *dA = D.up(arena.data(), arena.size());
    float *dx = D.up(x, n, 16);
    float *dxr = D.alloc<float>(n, 16);
    float *draw = D.fill<float>(n, 0, 16);
    float *dout = D.alloc<float>(n, 16);
    TCHECK(D.err);
    sx_block_kernel<<<dim3((T + 255) / 256, C / 8, B), 256>>>(dx, (int64_t)C * T, T, nullptr, dxr, C, T);
    SxPairArgs a{};
    a.xr = dxr;
    a.islope = a.mslope = slope;
    a.T = T;
    a.wp1 = reinterpret_cast<const u32x4 *>(dA + d1.w_off);
    a.wp2 = reinterpret_cast<const u32x4 *>(dA + d2.w_off);
    a.bias1 = d1.b_off >= 0 ? dA + d1.b_off : nullptr;
    a.bias2 = d2.b_off >= 0 ? dA + d2.b_off : nullptr;
    a.wscale1 = d1.wscale;
    a.wscale2 = d2.wscale;
    a.out_raw = draw;
    a.zeros = dA;
    a.C = C;
    a.K1 = d1.K; a.dil1 = d1.dil; a.pad1 = d1.padL;
    a.K2 = d2.K; a.dil2 = d2.dil; a.pad2 = d2.padL;
    a.div = 1.f;
    auto go = [&] { return launch_conv_sx_pair(a, d1.cfg, B, nullptr, chain != 0); };
    TCHECK(go());
    TCHECK(hipDeviceSynchronize());
    if (ms_out) TCHECK(time_launches(10, go, ms_out));
    sx_unblock_kernel<<<dim3((T + 255) / 256, C / 8, B), 256>>>(draw, nullptr, dout, C, T, 1);
    TCHECK(hipGetLastError());
    TCHECK(hipDeviceSynchronize());
    TCHECK(download(out, dout, n));
    return VITS_OK;
}

// conv_sx_pair_kernel with the argument set the generator's conv_sx_pair() gives it (include/vitsmi.h): SxPairArgs from
// sx_pair_args(), the generator's own filler, one launch_conv_sx_pair().  The raw output tensor starts as out_init (the ACC
// operand), else as zeros; what the launch does not write reads back unchanged.
int vits_test_conv_pair_sx_epi(int device_id, vits_test_conv_pair_sx_epi_args *p) {
    if (int rc = test_dev(device_id)) return rc;
    if (!p) return fail(nullptr, VITS_E_ARG, "no arguments");
    const auto bad = [](const char *why) { return fail(nullptr, VITS_E_ARG, "pair epilogue hook: %s", why); };
    const int B = p->B, C = p->C, T = p->T, K = p->K;
    if (B < 1 || C < 1 || T < 1 || K < 1 || p->dil1 < 1 || p->dil2 < 1 || !p->x || !p->w1 || !p->w2 || !p->out) return bad("bad shape or missing tensor");
    if (p->flags & ~(VITS_PAIR_EPI_ACC | VITS_PAIR_EPI_DIV)) return bad("unknown flag");
    if ((p->flags & VITS_PAIR_EPI_ACC) && !p->out_init) return bad("acc without out_init (the accumulate operand is the raw tensor's previous contents)");
    if (p->lens)
        for (int b = 0; b < B; b++)
            if (p->lens[b] < 0 || p->lens[b] > T) return bad("lens outside [0, T]");
    ConvDesc d1, d2;
    std::vector<float> arena;
    const TestPack o = sx_test_pack(SxPack::F16X2);
    std::string e = pack_test_conv(p->w1, p->b1, C, C, K, p->dil1, p->dil1 * (K - 1) / 2, 3, &d1, &arena, o);
    if (e.empty()) e = pack_test_conv(p->w2, p->b2, C, C, K, p->dil2, p->dil2 * (K - 1) / 2, 3, &d2, &arena, o);
    if (!e.empty()) return fail(nullptr, VITS_E_ARG, "%s", e.c_str());
    if (!d1.rawin || !d2.rawin || d1.cfg != d2.cfg || !sx_pair_supported(C, d1.cfg, d1.K, d1.dil, d2.K, d2.dil))
        return fail(nullptr, VITS_E_ARG, "this conv pair cannot run fused (C %d, kernel %d, dilations %d, %d)", C, K, p->dil1, p->dil2);
    const size_t n = (size_t)B * C * T;
    std::vector<int> l32(B);
    for (int b = 0; b < B; b++) l32[b] = p->lens ? (int)p->lens[b] : T;
    DevBufs D;
    float *dA = D.up(arena.data(), arena.size());
    float *dx = D.up(p->x, n, 16);
    float *dxr = D.alloc<float>(n, 16);
    float *dimg = p->out_init ? D.up(p->out_init, n, 16) : D.fill<float>(n, 0, 16);
    float *draw = D.alloc<float>(n, 16);
    float *dout = D.alloc<float>(n, 16);
    int *dlen = p->lens ? D.up(l32.data(), (size_t)B) : nullptr;
    TCHECK(D.err);
    const dim3 grid((T + 255) / 256, C / 8, B);
    sx_block_kernel<<<grid, 256>>>(dx, (int64_t)C * T, T, nullptr, dxr, C, T);
    sx_block_kernel<<<grid, 256>>>(dimg, (int64_t)C * T, T, nullptr, draw, C, T);
    TCHECK(hipGetLastError());
    const int kflags = ((p->flags & VITS_PAIR_EPI_ACC) ? EPI_ACC : 0) | ((p->flags & VITS_PAIR_EPI_DIV) ? EPI_DIV : 0);
    const SxRagged rag = dlen ? SxRagged{dlen, 0, 1} : SxRagged{nullptr, 0, 0};  // (utterance b's tensors end at lens[b] columns)
    const SxPairArgs a = sx_pair_args(d1, d2, dA, dA, dxr, T, draw, kflags, p->div == 0.f ? 1.f : p->div, p->slope, rag, nullptr);  // (pack_test_* reserve a zero page at offset 0)
    const bool name_was_on = g_launch_name_on;
    g_launch_name_on = true;
    g_launch_name[0] = 0;
    const hipError_t le = launch_conv_sx_pair(a, d1.cfg, B, nullptr, p->chain != 0);
    g_launch_name_on = name_was_on;
    if (le != hipSuccess) return fail(nullptr, VITS_E_DEVICE, "pair epilogue hook: launch_conv_sx_pair: %s", hipGetErrorString(le));
    TCHECK(hipDeviceSynchronize());
    std::snprintf(p->kernel, sizeof p->kernel, "%s", g_launch_name);
    p->BNo = 256 - (d2.K - 1) * d2.dil;
    sx_unblock_kernel<<<grid, 256>>>(draw, nullptr, dout, C, T, 1);
    TCHECK(hipGetLastError());
    TCHECK(hipDeviceSynchronize());
    TCHECK(download(p->out, dout, n));
    return VITS_OK;
}

// The identity behind split2h_pair_pk_mix (sx_split.hip.hpp), on the HOST in _Float16 / fmaf: for a value v (clamped to
// +-65504 as the split clamps it) and h0 = f16(v), the low plane in the two-rounding-free forms
//   old   f16((v - h0) * 2048)        fused   f16(fmaf(h0, -2048, v * 2048))
// Array form: both low planes' bits for x[0 .. n).  Sweep form: every fp32 bit pattern first, first + 1, .. (count of them):
// returns how many differ (two NaNs count as equal), *first_bad = the first such pattern.  No device is touched.
static inline void split_identity_one(float x, uint16_t *o, uint16_t *f) {
    const float v = std::fmin(std::fmax(x, -kF16Max), kF16Max);
    const _Float16 h0 = (_Float16)v;
    const _Float16 a = (_Float16)((v - (float)h0) * 2048.f);
    const _Float16 b = (_Float16)std::fmaf((float)h0, -2048.f, v * 2048.f);
    *o = __builtin_bit_cast(uint16_t, a);
    *f = __builtin_bit_cast(uint16_t, b);
}
int vits_test_split_identity(const float *x, int64_t n, uint16_t *h1_old, uint16_t *h1_fused) {
    if (!x || n < 0 || !h1_old || !h1_fused) return fail(nullptr, VITS_E_ARG, "split identity: missing array");
    for (int64_t i = 0; i < n; i++) split_identity_one(x[i], h1_old + i, h1_fused + i);
    return VITS_OK;
}
int64_t vits_test_split_identity_sweep(uint32_t first, uint64_t count, uint32_t *first_bad) {
    int64_t bad = 0;
    for (uint64_t k = 0; k < count; k++) {
        const uint32_t bits = first + (uint32_t)k;
        uint16_t o, f;
        split_identity_one(__builtin_bit_cast(float, bits), &o, &f);
        const bool nan_o = (o & 0x7fffu) > 0x7c00u, nan_f = (f & 0x7fffu) > 0x7c00u;
        if (o != f && !(nan_o && nan_f)) {
            if (bad == 0 && first_bad) *first_bad = bits;
            bad++;
        }
    }
    return bad;
}

// split_forms_kernel (test_dev.hip.hpp) on n values (n even): form 0 = split2h_pair_pk, 1 = conv_sx_pair_kernel's split.
int vits_test_split_forms(int device_id, const float *x, int n, float slope, int form, uint16_t *h0, uint16_t *h1, float *pk, float *rec) {
    if (int rc = test_dev(device_id)) return rc;
    if (!x || n < 2 || (n & 1) || !(slope > 0.f) || slope > 1.f || form < 0 || form > 1 || !h0 || !h1 || !pk || !rec)
        return fail(nullptr, VITS_E_ARG, "split forms hook: n even and >= 2, 0 < slope <= 1, form 0 or 1, every output given");
    DevBufs D;
    float *dx = D.up(x, (size_t)n);
    uint16_t *d0 = D.alloc<uint16_t>((size_t)n), *d1 = D.alloc<uint16_t>((size_t)n);
    float *dpk = D.alloc<float>((size_t)n / 2), *drec = D.alloc<float>((size_t)n);
    TCHECK(D.err);
    const unsigned blocks = (unsigned)((n / 2 + 255) / 256);
    if (form == 0) split_forms_kernel<0><<<blocks, 256>>>(dx, n, slope, 1.f / slope, d0, d1, dpk, drec);
    else split_forms_kernel<1><<<blocks, 256>>>(dx, n, slope, 1.f / slope, d0, d1, dpk, drec);
    TCHECK(hipGetLastError());
    TCHECK(hipDeviceSynchronize());
    TCHECK(download(h0, d0, (size_t)n));
    TCHECK(download(h1, d1, (size_t)n));
    TCHECK(download(pk, dpk, (size_t)n / 2));
    TCHECK(download(rec, drec, (size_t)n));
    return VITS_OK;
}

int vits_bench_conv1d_sx(int device_id, int B, int Cin, int Cout, int T, int K, int dil, int dbg, int iters,
                         float *ms_out) {
    if (int rc = test_dev(device_id)) return rc;
    std::vector<float> w((size_t)Cout * Cin * K), x((size_t)B * Cin * T);
    bench_fill(w, x);
    ConvDesc d;
    std::vector<float> arena;
    // bit 6: one fp16 plane, one product (VITSMI_GEN_PRECISION=f16); bit 7: two fp16 planes
    TestPack o = sx_test_pack((dbg & 64) ? SxPack::F16X1 : ((dbg & 128) ? SxPack::F16X2 : SxPack::BF16X3));
    o.sx.no_s16 = (dbg & (1 | 2 | 16 | 256)) != 0;  // ablation / cycle-breakdown builds exist for the 32x32x16 loop only
    std::string e = pack_test_conv(w.data(), nullptr, Cin, Cout, K, dil, dil * (K - 1) / 2, 3, &d, &arena, o);
    if (!e.empty()) return fail(nullptr, VITS_E_ARG, "%s", e.c_str());
    const size_t nx = x.size(), no = (size_t)B * Cout * T;
    DevBufs D;
    float *dA = D.up(arena.data(), arena.size());
    float *dx = D.up(x.data(), nx);
    uint16_t *dxp = D.alloc<uint16_t>(nx * 3);
    float *draw = D.alloc<float>(no);
    float *dres = D.fill<float>(no);
    uint16_t *dop = D.alloc<uint16_t>(no * 3);
    // per-step cycle breakdown (128x128 tile only), returned in ms_out[3..8]
    unsigned long long *dprof = (dbg & 16) ? D.fill<unsigned long long>(8) : nullptr;
    TCHECK(D.err);
    sx_split_planes_kernel<<<dim3((T + 255) / 256, Cin / 8, B), 256>>>(dx, (int64_t)Cin * T, T, nullptr, dxp, Cin, T,
                                                                       d.h1 ? 2 : (d.f16 ? 1 : 0));
    SxArgs a = sx_args(d, dA, dA, T);  // (pack_test_* reserve a zero page at offset 0)
    a.xp = reinterpret_cast<const u32x4 *>(dxp);
    a.out_pl = dop;  // as the generator's inner convs: planes out
    a.oslope2 = 0.1f;
    a.flags = ((dbg & 1) ? DBG_NO_DMA : 0) | ((dbg & 2) ? DBG_NO_EPI : 0);
    if (dbg & 8) {  // residual epilogue with raw + planes outputs (ResBlock tail)
        a.flags |= EPI_RES;
        if (d.h1) {  // (single-plane mode: plane in, residual from a plane, plane out - the ResBlock tail of that mode)
            a.res_pl = reinterpret_cast<const uint16_t *>(dres);
            a.res_unslope = 10.f;
        } else {
            a.res = dres;
            a.out_raw = draw;
        }
    }
    if (d.rawin) {  // <= 64 input channels: as the generator runs such layers: fp32 raw in (lrelu on load), raw out
        a.xr = dx;
        a.islope = 0.1f;
        a.out_pl = nullptr;
        a.out_raw = draw;
    }
    a.prof = dprof;
    auto go = [&] { return launch_conv_sx(a, d.cfg, B, nullptr, d.rawin, d.h1 ? 1 : (d.f16 ? 2 : 6)); };
    for (int i = 0; i < 2; i++) TCHECK(go());
    TCHECK(hipDeviceSynchronize());
    if (dprof) TCHECK(hipMemset(dprof, 0, 64));
    float ms = 0.f;
    TCHECK(time_launches(iters, go, &ms));
    if (ms_out) {
        ms_out[0] = ms;
        ms_out[1] = (float)d.cfg;
        ms_out[2] = 0.f;
        if (dprof) {
            unsigned long long hp[8];
            TCHECK(download(hp, dprof, 8));
            for (int i = 0; i < 5; i++) ms_out[3 + i] = hp[5] ? (float)((double)hp[i] / (double)hp[5]) : 0.f;  // per step
            ms_out[2] = hp[7] ? (float)((double)hp[6] / (double)hp[7] * 0.1) : 0.f;  // shader clock, GHz
        }
    }
    return VITS_OK;
}

int vits_test_attention(int device_id, const float *qkv, int B, int C, int T, int n_heads, const float *rel_k,
                        const float *rel_v, int window, const int64_t *lens, float *out) {
    if (int rc = test_dev(device_id)) return rc;
    if (window > 4 || C % n_heads) return fail(nullptr, VITS_E_ARG, "bad attention test arguments");
    int dk = C / n_heads;
    if (dk > kAttMaxHeadWidth) return fail(nullptr, VITS_E_ARG, "attention head width %d > %d is unsupported", dk, kAttMaxHeadWidth);
    size_t nq = (size_t)B * 3 * C * T, no = (size_t)B * C * T, nr = (size_t)(2 * window + 1) * dk;
    std::vector<int> l32(B);
    for (int b = 0; b < B; b++) l32[b] = (int)lens[b];
    DevBufs D;
    float *dq = D.up(qkv, nq);
    float *dout = D.alloc<float>(no);
    float *drk = D.up(rel_k, nr);
    float *drv = D.up(rel_v, nr);
    int *dlen = D.up(l32.data(), (size_t)B);
    TCHECK(D.err);
    launch_attention(nullptr, B, T, n_heads, dk, window, dq, dout, drk, drv, dlen, C);
    TCHECK(hipGetLastError());
    TCHECK(hipDeviceSynchronize());
    TCHECK(download(out, dout, no));
    return VITS_OK;
}

// ... the 16x16x32 f16x3 kernel (kernel = 1) or the fp32-MFMA one (0) with timing: the q | k | v tensor is split into
// operand planes on the device first (what the q|k|v conv's epilogue does in the pipeline); out_planes (optional) receives the
// output's operand planes [B][3][C/8][T][8]; reps > 0: ms_out[0] = mean launch duration over reps launches (HIP events).
int vits_test_attention16(int device_id, const float *qkv, int B, int C, int T, int n_heads, const float *rel_k,
                          const float *rel_v, int window, const int64_t *lens, float *out, uint16_t *out_planes, int kernel,
                          int reps, float *ms_out) {
    if (int rc = test_dev(device_id)) return rc;
    if (window > 4 || C % n_heads || C % 8) return fail(nullptr, VITS_E_ARG, "bad attention test arguments");
    int dk = C / n_heads;
    if (kernel == 1 && !(dk % 32 == 0 && dk <= 96)) return fail(nullptr, VITS_E_ARG, "attention16 needs a head width of 32, 64 or 96");
    if (dk > kAttMaxHeadWidth) return fail(nullptr, VITS_E_ARG, "attention head width %d > %d is unsupported", dk, kAttMaxHeadWidth);
    size_t nq = (size_t)B * 3 * C * T, no = (size_t)B * C * T, nr = (size_t)(2 * window + 1) * dk;
    std::vector<int> l32(B);
    for (int b = 0; b < B; b++) l32[b] = (int)lens[b];
    DevBufs D;
    float *dq = D.up(qkv, nq);
    uint16_t *dqp = D.alloc<uint16_t>(nq * 3);
    uint16_t *dop = D.fill<uint16_t>(no * 3, 0xff);
    unsigned *dpk = D.fill<unsigned>((size_t)kSxPeakSlots * kSxPeakStride);
    float *dout = D.fill<float>(no, 0xff);
    float *drk = D.up(rel_k, nr);
    float *drv = D.up(rel_v, nr);
    int *dlen = D.up(l32.data(), (size_t)B);
    unsigned long long *dprof = nullptr;
    const int prof_wgs = ((n_heads * B + 7) / 8) * 8 * ((T + 63) / 64);
#if ATT16_PROF
    dprof = D.fill<unsigned long long>((size_t)prof_wgs * 4);
#endif
    TCHECK(D.err);
    sx_split_planes_kernel<<<dim3((T + 255) / 256, 3 * C / 8, B), 256>>>(dq, (int64_t)3 * C * T, T, nullptr, dqp, 3 * C, T, 1, dpk);
    auto go = [&] {
        if (kernel == 1) (void)launch_attention16(nullptr, B, T, n_heads, dk, window, dqp, dout, dop, drk, drv, dlen, C, dpk, dprof);
        else launch_attention(nullptr, B, T, n_heads, dk, window, dq, dout, drk, drv, dlen, C, dk % 8 == 0 ? dop : nullptr, dpk);
        return hipSuccess;
    };
    go();
    TCHECK(hipGetLastError());
    TCHECK(hipDeviceSynchronize());
    if (reps > 0 && ms_out) TCHECK(time_launches(reps, go, ms_out));
    if (dprof && kernel == 1) {  // ATT16_PROF builds: where a workgroup's time goes (shader-clock cycles, means over the launch)
        std::vector<unsigned long long> hp((size_t)prof_wgs * 4);
        TCHECK(download(hp.data(), dprof, hp.size()));
        double d[3] = {0, 0, 0};
        unsigned long long t0 = ~0ull, t1 = 0;
        int n = 0;
        for (int w = 0; w < prof_wgs; w++) {
            if (!hp[w * 4 + 3]) continue;
            for (int k = 0; k < 3; k++) d[k] += (double)(hp[w * 4 + k + 1] - hp[w * 4 + k]);
            t0 = hp[w * 4] < t0 ? hp[w * 4] : t0;
            t1 = hp[w * 4 + 3] > t1 ? hp[w * 4 + 3] : t1;
            n++;
        }
        if (n) std::fprintf(stderr, "att16 stamps B=%d T=%d: %d workgroups; cycles prologue %.0f loop %.0f epilogue %.0f; first start -> last end %llu\n",
                            B, T, n, d[0] / n, d[1] / n, d[2] / n, t1 - t0);
    }
    TCHECK(download(out, dout, no));
    if (out_planes) TCHECK(download(out_planes, dop, no * 3));
    return VITS_OK;
}

// ... either kernel in the form and instantiation the caller names: which outputs the launch writes (the pipeline's
// attention16 launch writes planes only), stages / query tiles / key halves, q | k | v planes split here or given.  Both output
// buffers start as 0xff bytes and come back whole, so what a launch did not write shows.  A (dk, ns, qt, kh) without a
// compiled instantiation is refused: nothing is rounded to a neighbour.
int vits_test_attention_form(int device_id, vits_test_attention_form_args *p) {
    if (int rc = test_dev(device_id)) return rc;
    if (!p) return fail(nullptr, VITS_E_ARG, "no attention test arguments");
    const int B = p->B, C = p->C, T = p->T, n_heads = p->n_heads, window = p->window;
    if (B <= 0 || C <= 0 || T <= 0 || n_heads <= 0 || window < 0 || !p->rel_k || !p->rel_v || !p->lens)
        return fail(nullptr, VITS_E_ARG, "bad attention test arguments");
    if (window > 4) return fail(nullptr, VITS_E_ARG, "attention window %d > 4 is unsupported", window);
    if (C % n_heads) return fail(nullptr, VITS_E_ARG, "%d channels do not divide into %d heads", C, n_heads);
    const int dk = C / n_heads;
    if (dk > kAttMaxHeadWidth) return fail(nullptr, VITS_E_ARG, "attention head width %d > %d is unsupported", dk, kAttMaxHeadWidth);
    const bool k16 = p->kernel == 16;
    if (!k16 && p->kernel != 32) return fail(nullptr, VITS_E_ARG, "kernel must be 16 (attention16) or 32 (the fp32-MFMA kernel), not %d", p->kernel);
    if (!p->want_out && !p->want_planes) return fail(nullptr, VITS_E_ARG, "a launch that writes neither output");
    if ((p->want_out && !p->out) || (p->want_planes && !p->out_planes)) return fail(nullptr, VITS_E_ARG, "a wanted output has no buffer");
    if (p->want_planes && C % 8) return fail(nullptr, VITS_E_ARG, "output planes need a multiple of 8 channels, not %d", C);
    if (k16) {
        if (!(dk == 32 || dk == 64 || dk == 96)) return fail(nullptr, VITS_E_ARG, "attention16 needs a head width of 32, 64 or 96, not %d", dk);
        if (p->kh) return fail(nullptr, VITS_E_ARG, "attention16 has no key halves (kh = %d)", p->kh);
        const int ns = p->ns, qt = p->qt;
        // the compiled instantiations: <1, 3, 1>, <2, 3, 1>, <3, {2, 3, 4}, 1>, <3, {2, 3}, 2>
        const bool have = dk < 96 ? (ns == 0 || ns == 3) && (qt == 0 || qt == 1)
                                  : qt == 2 ? (ns == 0 || ns == 2 || ns == 3) : (qt == 0 || qt == 1) && (ns == 0 || (ns >= 2 && ns <= 4));
        if (!have) return fail(nullptr, VITS_E_ARG, "no attention16 instantiation <%d, %d, %d>", dk / 32, ns, qt);
        if (!p->qkv && !p->qkv_planes) return fail(nullptr, VITS_E_ARG, "neither q|k|v nor its planes given");
    } else {
        if (p->ns || p->qt) return fail(nullptr, VITS_E_ARG, "the fp32 kernel has no stages or query tiles (ns = %d, qt = %d)", p->ns, p->qt);
        if (p->kh < 0 || p->kh > 2) return fail(nullptr, VITS_E_ARG, "no fp32 attention instantiation with %d key halves", p->kh);
        if (!p->want_out) return fail(nullptr, VITS_E_ARG, "the fp32 kernel always writes its fp32 output");
        if (p->want_planes && dk % 8) return fail(nullptr, VITS_E_ARG, "the fp32 kernel's planes need a head width that is a multiple of 8, not %d", dk);
        if (!p->qkv || p->qkv_planes) return fail(nullptr, VITS_E_ARG, "the fp32 kernel reads q|k|v as fp32");
    }
    const size_t nq = (size_t)B * 3 * C * T, no = (size_t)B * C * T, nr = (size_t)(2 * window + 1) * dk;
    std::vector<int> l32(B);
    for (int b = 0; b < B; b++) {
        if (p->lens[b] < 0) return fail(nullptr, VITS_E_ARG, "lens[%d] = %lld", b, (long long)p->lens[b]);
        l32[b] = (int)std::min<int64_t>(p->lens[b], INT_MAX);
    }
    DevBufs D;
    float *dq = p->qkv && !p->qkv_planes ? D.up(p->qkv, nq) : nullptr;
    uint16_t *dqp = nullptr;
    if (k16) dqp = p->qkv_planes ? D.up(p->qkv_planes, nq * 3) : D.alloc<uint16_t>(nq * 3);
    uint16_t *dop = C % 8 == 0 ? D.fill<uint16_t>(no * 3, 0xff) : nullptr;
    unsigned *dpk = D.fill<unsigned>((size_t)kSxPeakSlots * kSxPeakStride);
    float *dout = D.fill<float>(no, 0xff);
    float *drk = D.up(p->rel_k, nr);
    float *drv = D.up(p->rel_v, nr);
    int *dlen = D.up(l32.data(), (size_t)B);
    TCHECK(D.err);
    if (k16 && !p->qkv_planes) {
        sx_split_planes_kernel<<<dim3((T + 255) / 256, 3 * C / 8, B), 256>>>(dq, (int64_t)3 * C * T, T, nullptr, dqp, 3 * C, T, 1, dpk);
        TCHECK(hipGetLastError());
        // (the split has left the peak of q | k | v in the slots: the attention launch starts from zeros)
        TCHECK(hipMemsetAsync(dpk, 0, (size_t)kSxPeakSlots * kSxPeakStride * sizeof(unsigned), nullptr));
    }
    const bool name_was_on = g_launch_name_on;
    g_launch_name_on = true;
    g_launch_name[0] = 0;
    hipError_t le = hipSuccess;
    if (k16)
        le = launch_attention16(nullptr, B, T, n_heads, dk, window, dqp, p->want_out ? dout : nullptr, p->want_planes ? dop : nullptr,
                                drk, drv, dlen, C, dpk, nullptr, p->ns, p->qt);
    else
        launch_attention(nullptr, B, T, n_heads, dk, window, dq, dout, drk, drv, dlen, C, p->want_planes ? dop : nullptr, dpk, p->kh);
    g_launch_name_on = name_was_on;
    TCHECK(le);
    std::snprintf(p->kernel_name, sizeof p->kernel_name, "%s", g_launch_name);
    TCHECK(hipGetLastError());
    TCHECK(hipDeviceSynchronize());
    if (p->out) TCHECK(download(p->out, dout, no));
    if (p->out_planes && dop) TCHECK(download(p->out_planes, dop, no * 3));
    {
        std::vector<unsigned> slots((size_t)kSxPeakSlots * kSxPeakStride);
        TCHECK(download(slots.data(), dpk, slots.size()));
        unsigned top = 0;
        for (int s = 0; s < kSxPeakSlots; s++) top = std::max(top, slots[(size_t)s * kSxPeakStride]);
        std::memcpy(&p->peak, &top, 4);
    }
    return VITS_OK;
}

// The resampler by value: what both hooks share - the plan's table on the device, the rows' valid input samples
// (lens, clipped to [0, S]) and output sample counts.
namespace {
struct ResampleTest {
    ResampleDev dev;
    std::vector<int> n_in, n_out;
    int *d_n_in = nullptr, *d_n_out = nullptr;
    int64_t n_max = 0;
};
int resample_test_setup(DevBufs &D, const int64_t *lens, int B, int S, int in_rate, int out_rate, ResampleTest &t) {
    if (!lens || B <= 0 || S <= 0) return fail(nullptr, VITS_E_ARG, "bad resampler test arguments");
    const std::string e = resample_plan(in_rate, out_rate, t.dev.plan);
    if (!e.empty()) return fail(nullptr, VITS_E_ARG, "%s", e.c_str());
    const ResamplePlan &p = t.dev.plan;
    if (p.count(S) > INT_MAX) return fail(nullptr, VITS_E_ARG, "%d samples are %lld at %d Hz", S, (long long)p.count(S), out_rate);
    t.dev.Kp = resample_pitch(p);
    std::vector<float> tab((size_t)p.L * t.dev.Kp);
    resample_table(p, tab.data(), t.dev.Kp);
    t.dev.table = D.up(tab.data(), tab.size());
    for (int b = 0; b < B; b++) {
        const int64_t n = lens[b] < 0 ? 0 : (lens[b] > S ? S : lens[b]);
        t.n_in.push_back((int)n);
        t.n_out.push_back((int)p.count(n));
        t.n_max = p.count(n) > t.n_max ? p.count(n) : t.n_max;
    }
    t.d_n_in = D.up(t.n_in.data(), (size_t)B);
    t.d_n_out = D.up(t.n_out.data(), (size_t)B);
    return VITS_OK;
}
}  // namespace

int vits_test_resample(int device_id, const float *x, const int64_t *lens, int B, int S, int in_rate, int out_rate, float *y,
                       int64_t S_out) {
    if (int rc = test_dev(device_id)) return rc;
    if (!x || !y) return fail(nullptr, VITS_E_ARG, "bad resampler test arguments");
    DevBufs D;
    ResampleTest t;
    if (int rc = resample_test_setup(D, lens, B, S, in_rate, out_rate, t)) return rc;
    if (S_out < t.n_max || S_out < 1 || S_out > INT_MAX)
        return fail(nullptr, VITS_E_ARG, "S_out = %lld, the longest row has %lld output samples", (long long)S_out, (long long)t.n_max);
    float *dx = D.up(x, (size_t)B * S);
    float *dy = D.fill<float>((size_t)B * S_out, 0xff);
    TCHECK(D.err);
    ResampleArgs a = resample_args(t.dev);
    a.x = dx;
    a.x_pitch = S;
    a.x_n = S;
    a.n_in = t.d_n_in;
    a.n_out = t.d_n_out;
    a.y = dy;
    a.y_pitch = S_out;
    a.n_hi = (int)S_out;
    TCHECK(launch_resample(a, B, /*piece=*/false, nullptr));
    TCHECK(hipDeviceSynchronize());
    TCHECK(download(y, dy, (size_t)B * S_out));
    return VITS_OK;
}

// The time warp and the glide by value: the rows' records from the caller's segments, the pipeline's launch.
extern "C++" {
namespace {
// The front matter of every warp hook, row by row: seg_first ascends, the row's records pass the family's `fault`, its valid
// input is counts[b] clamped to [0, S] -> n_in[b]; then per_row(b, the row's record count) - what the hook checks of a row
// besides, 0 or its failure.  The first thing wrong is the answer.
template <class Seg, class Fault, class PerRow>
int warp_test_rows(const Seg *segs, const int32_t *seg_first, const int64_t *counts, int B, int S, Fault fault, std::vector<int64_t> &n_in,
                   PerRow per_row) {
    n_in.assign((size_t)B, 0);
    for (int b = 0; b < B; b++) {
        const int32_t ns = seg_first[b + 1] - seg_first[b];
        if (ns < 0 || (ns > 0 && !segs)) return fail(nullptr, VITS_E_ARG, "row %d: seg_first is not ascending", b);
        const std::string e = fault(segs + seg_first[b], ns);
        if (!e.empty()) return fail(nullptr, VITS_E_ARG, "row %d: %s", b, e.c_str());
        n_in[(size_t)b] = counts[b] < 0 ? 0 : (counts[b] > S ? S : counts[b]);
        if (int rc = per_row(b, ns)) return rc;
    }
    return 0;
}
template <class Seg, class Fault>
int warp_test_rows(const Seg *segs, const int32_t *seg_first, const int64_t *counts, int B, int S, Fault fault, std::vector<int64_t> &n_in) {
    return warp_test_rows(segs, seg_first, counts, B, S, fault, n_in, [](int, int32_t) { return 0; });
}

// G, the records, the rows and x [B][S] on the device, y poisoned; output samples [n_lo, n_hi) of every row through the
// pipeline's launch into y [B][n_hi - n_lo]
template <class Seg, class Row>
int warp_test_launch(DevBufs &D, const Seg *segs, size_t n_segs, const std::vector<Row> &rows, const float *x, int B, int S, int n_lo, int n_hi,
                     float *y) {
    std::vector<float> G(kWarpTable);
    warp_table(G.data());
    const Seg none{};
    WarpArgsT<Seg, Row> a{};
    a.segs = D.up(n_segs ? segs : &none, n_segs ? n_segs : 1);
    a.rows = D.up(rows.data(), rows.size());
    a.G = D.up(G.data(), G.size());
    a.x = D.up(x, (size_t)B * S);
    a.x_pitch = S;
    const int64_t W = (int64_t)n_hi - n_lo;
    float *dy = D.fill<float>((size_t)B * W, 0xff);
    a.y = dy;
    a.y_pitch = W;
    a.n_lo = n_lo;
    a.n_hi = n_hi;
    TCHECK(D.err);
    TCHECK(launch_warp_tile(a, B, nullptr));
    TCHECK(hipDeviceSynchronize());
    TCHECK(download(y, dy, (size_t)B * W));
    return VITS_OK;
}

template <class Seg, class Fault>
int test_warp_as(int device_id, const float *x, const int64_t *counts, int B, int S, const Seg *segs, const int32_t *seg_first,
                 float *y, int S_w, Fault fault) {
    if (int rc = test_dev(device_id)) return rc;
    if (!x || !y || !counts || !seg_first || B <= 0 || S <= 0 || S_w < 1) return fail(nullptr, VITS_E_ARG, "bad warp test arguments");
    if (seg_first[0] != 0) return fail(nullptr, VITS_E_ARG, "seg_first[0] = %d, not 0", (int)seg_first[0]);
    std::vector<int64_t> n_in;
    if (int rc = warp_test_rows(segs, seg_first, counts, B, S, fault, n_in)) return rc;
    std::vector<WarpRow> rows;
    const int64_t need = warp_rows(segs, seg_first, n_in.data(), B, rows);
    if (S_w < need) return fail(nullptr, VITS_E_ARG, "S_w = %d, the longest row has %lld output samples", S_w, (long long)need);
    DevBufs D;
    return warp_test_launch(D, segs, (size_t)seg_first[B], rows, x, B, S, 0, S_w, y);
}
}  // namespace
}  // extern "C++"

int vits_test_warp(int device_id, const float *x, const int64_t *counts, int B, int S, const vits_warp_seg *segs, const int32_t *seg_first,
                   float *y, int S_w) {
    return test_warp_as(device_id, x, counts, B, S, segs, seg_first, y, S_w, warp_segs_fault);
}

int vits_test_glide(int device_id, const float *x, const int64_t *counts, int B, int S, const vits_glide_seg *segs, const int32_t *seg_first,
                    float *y, int S_w) {
    return test_warp_as(device_id, x, counts, B, S, segs, seg_first, y, S_w, glide_segs_fault);
}

// The wide kernels ("pitch at an output rate") by value: the caller's records under the folded limits, a pair of rates per row
// (in_rates[b] -> out_rates[b]; 0 or in_rates[b]: native), output samples [n_lo, n_hi) of every row through the pipeline's launch into y [B][n_hi - n_lo].
// A row without a record is an identity row: ceil(n_b * L / M) samples by the resampler's rule.
extern "C++" {
namespace {
template <class Seg, class Fault>
int test_warp_rate_as(int device_id, const float *x, const int64_t *counts, int B, int S, const Seg *segs, const int32_t *seg_first,
                      const int32_t *in_rates, const int32_t *out_rates, int n_lo, int n_hi, float *y, Fault fault) {
    if (int rc = test_dev(device_id)) return rc;
    if (!x || !y || !counts || !seg_first || !in_rates || !out_rates || B <= 0 || S <= 0 || n_lo < 0 || n_hi <= n_lo)
        return fail(nullptr, VITS_E_ARG, "bad warp test arguments");
    if (seg_first[0] != 0) return fail(nullptr, VITS_E_ARG, "seg_first[0] = %d, not 0", (int)seg_first[0]);
    std::vector<int64_t> n_in, L((size_t)B, 1), M((size_t)B, 1);
    std::vector<ResamplePlan> plans((size_t)B);
    const auto rates = [&](int b, int32_t ns) {  // the row's pair of rates -> its plan
        const int in_rate = in_rates[b];
        if (out_rates[b] == 0 || out_rates[b] == in_rate) return 0;
        const std::string pe = resample_plan(in_rate, out_rates[b], plans[(size_t)b]);
        if (!pe.empty()) return fail(nullptr, VITS_E_ARG, "row %d: %s", b, pe.c_str());
        L[(size_t)b] = plans[(size_t)b].L;
        M[(size_t)b] = plans[(size_t)b].M;
        if (ns > 0 && !warp_rate_ok(L[(size_t)b], M[(size_t)b]))
            return fail(nullptr, VITS_E_ARG, "row %d: pitch at %d -> %d Hz: the ratio of the rates lies outside [1/4, 4]", b, in_rate, (int)out_rates[b]);
        return 0;
    };
    if (int rc = warp_test_rows(segs, seg_first, counts, B, S, fault, n_in, rates)) return rc;
    std::vector<WarpRateRow> rows;
    const int64_t need = warp_rate_rows(segs, seg_first, n_in.data(), L.data(), M.data(), B, rows);
    if (need > INT_MAX) return fail(nullptr, VITS_E_ARG, "the longest row has %lld output samples", (long long)need);
    DevBufs D;
    for (int b = 0; b < B; b++) {  // the table of every resampled row (rows at one rate share it)
        if (!plans[(size_t)b].on()) continue;
        WarpRateRow &r = rows[(size_t)b];
        r.Kp = resample_pitch(plans[(size_t)b]);
        r.K = (int32_t)plans[(size_t)b].K;
        for (int q = 0; q < b && !r.table; q++)
            if (out_rates[q] == out_rates[b] && in_rates[q] == in_rates[b]) r.table = rows[(size_t)q].table;
        if (r.table) continue;
        std::vector<float> t((size_t)r.L * r.Kp);
        resample_table(plans[(size_t)b], t.data(), r.Kp);
        r.table = D.up(t.data(), t.size());
    }
    return warp_test_launch(D, segs, (size_t)seg_first[B], rows, x, B, S, n_lo, n_hi, y);
}
}  // namespace
}  // extern "C++"

int vits_test_warp_rate(int device_id, const float *x, const int64_t *counts, int B, int S, const vits_warp_seg *segs, const int32_t *seg_first,
                        const int32_t *in_rates, const int32_t *out_rates, int n_lo, int n_hi, float *y) {
    return test_warp_rate_as(device_id, x, counts, B, S, segs, seg_first, in_rates, out_rates, n_lo, n_hi, y, warp_rate_segs_fault);
}

int vits_test_glide_rate(int device_id, const float *x, const int64_t *counts, int B, int S, const vits_glide_seg *segs, const int32_t *seg_first,
                         const int32_t *in_rates, const int32_t *out_rates, int n_lo, int n_hi, float *y) {
    return test_warp_rate_as(device_id, x, counts, B, S, segs, seg_first, in_rates, out_rates, n_lo, n_hi, y, glide_rate_segs_fault);
}

// Streamed pitch by value: the input cut at piece_bounds (increasing piece ends, the last one S), every piece through the
// pipeline's stage (warp_run_begin / _piece / _window) on the pipeline's walk; n_cap is warp_stream_cap of the longest piece.
// With a pair of rates ("pitch at an output rate") the wide stage: the same walk over a folded plan at ONE pair of rates - what a
// chunked run has -, n_cap = warp_stream_cap(longest piece, S_w, the plan's least step, its largest Kh).
extern "C++" {
namespace {
// "" or what is wrong with the piece ends; longest: the longest piece
int piece_bounds_check(const int64_t *piece_bounds, int n_pieces, int S, int64_t &longest) {
    longest = 0;
    for (int i = 0; i < n_pieces; i++) {
        const int64_t lo = i ? piece_bounds[i - 1] : 0;
        if (piece_bounds[i] <= lo || piece_bounds[i] > S) return fail(nullptr, VITS_E_ARG, "piece_bounds[%d] = %lld does not ascend within (0, %d]", i, (long long)piece_bounds[i], S);
        longest = piece_bounds[i] - lo > longest ? piece_bounds[i] - lo : longest;
    }
    if (piece_bounds[n_pieces - 1] != S) return fail(nullptr, VITS_E_ARG, "the last piece ends at %lld, not at S = %d", (long long)piece_bounds[n_pieces - 1], S);
    return 0;
}

// The planned run through the pipeline's stage on the pipeline's walk of a poisoned buffer: every piece of x [B][S] joins the
// history, every window it completes is copied into y [B][S_w].  Returns the number of windows.
int walk_warp_pieces(WarpRun &run, DevBufs &D, const float *x, int B, int S, int64_t n_cap, const int64_t *piece_bounds, int n_pieces, float *y,
                     int S_w, int64_t *ranges, int max_ranges) {
    std::vector<float> G(kWarpTable);
    warp_table(G.data());
    const float *dG = D.up(G.data(), G.size());
    const float *dx = D.up(x, (size_t)B * S);
    const auto walk = [&](Carver &cv) { return carve_warp_stream(cv, B, S, n_cap, run.n_segs(), run.row_bytes()); };
    const size_t bytes = carved_bytes(walk);
    Carver cv(D.fill<unsigned char>(bytes, 0xff), bytes);  // (poisoned: what a window must not read is NaN)
    TCHECK(D.err);
    const WarpStreamBufs wb = walk(cv);
    if (!cv.fits()) return fail(nullptr, VITS_E_NOMEM, "stream walk carved %zu of %zu bytes", cv.used, cv.cap);
    TCHECK(warp_run_begin(run, wb, dG, n_cap, B, nullptr, nullptr));
    std::vector<float> piece((size_t)B * n_cap);
    std::memset(y, 0, (size_t)B * S_w * sizeof(float));
    int calls = 0;
    for (int i = 0; i < n_pieces; i++) {
        const int64_t f0 = i ? piece_bounds[i - 1] : 0, n = piece_bounds[i] - f0;
        TCHECK(warp_run_piece(run, dx + f0, S, f0, n, i == n_pieces - 1, B, nullptr));
        for (;;) {
            const float *dy = nullptr;
            int64_t ef = 0, en = 0;
            int launches = 0;
            TCHECK(warp_run_window(run, B, nullptr, dy, ef, en, launches));
            if (en <= 0) break;
            TCHECK(hipDeviceSynchronize());
            TCHECK(download(piece.data(), dy, (size_t)B * en));
            for (int b = 0; b < B; b++) std::memcpy(y + (size_t)b * S_w + ef, piece.data() + (size_t)b * en, (size_t)en * sizeof(float));
            if (ranges && calls < max_ranges) {
                ranges[2 * calls] = ef;
                ranges[2 * calls + 1] = en;
            }
            calls++;
        }
    }
    TCHECK(hipDeviceSynchronize());
    return calls;
}

// rates: nullptr - the native stage -, or {in_rate, out_rate} - the folded one (out_rate 0 or in_rate: at the native rate)
template <class Seg, class Fault>
int test_warp_pieces_as(int device_id, const float *x, const int64_t *counts, int B, int S, const Seg *segs, const int32_t *seg_first,
                        const int *rates, const int64_t *piece_bounds, int n_pieces, float *y, int S_w, int64_t *ranges, int max_ranges,
                        Fault fault, std::vector<Seg> WarpRun::*mine) {
    if (int rc = test_dev(device_id)) return rc;
    if (!x || !y || !counts || !seg_first || !piece_bounds || B <= 0 || S <= 0 || S_w < 1 || n_pieces < 1)
        return fail(nullptr, VITS_E_ARG, "bad warp test arguments");
    if (seg_first[0] != 0) return fail(nullptr, VITS_E_ARG, "seg_first[0] = %d, not 0", (int)seg_first[0]);
    int64_t longest = 0;
    if (int rc = piece_bounds_check(piece_bounds, n_pieces, S, longest)) return rc;
    ResamplePlan plan;
    if (rates && rates[1] != 0 && rates[1] != rates[0]) {
        const std::string pe = resample_plan(rates[0], rates[1], plan);
        if (!pe.empty()) return fail(nullptr, VITS_E_ARG, "%s", pe.c_str());
        if (seg_first[B] > 0 && !warp_rate_ok(plan.L, plan.M))
            return fail(nullptr, VITS_E_ARG, "pitch at %d -> %d Hz: the ratio of the rates lies outside [1/4, 4]", rates[0], rates[1]);
    }
    std::vector<int64_t> n_in;
    if (int rc = warp_test_rows(segs, seg_first, counts, B, S, fault, n_in)) return rc;
    WarpRun run;
    run.glide = std::is_same_v<Seg, vits_glide_seg>;
    run.folded = rates != nullptr;
    (run.*mine).assign(segs, segs + seg_first[B]);
    run.first.assign(seg_first, seg_first + B + 1);
    if (rates) {
        const std::vector<int64_t> L((size_t)B, plan.L), M((size_t)B, plan.M);
        run.S_w = warp_rate_rows(segs, seg_first, n_in.data(), L.data(), M.data(), B, run.rrows);
    } else
        run.S_w = warp_rows(segs, seg_first, n_in.data(), B, run.rows);
    if (S_w != run.S_w) return fail(nullptr, VITS_E_ARG, "S_w = %d, the rows give %lld", S_w, (long long)run.S_w);
    int64_t min_step = kWarpMinStep;
    warp_run_visit(run, [&](auto &sg, auto &rows) { warp_plan_extent(sg.data(), rows, run.half, min_step); });
    const int64_t n_cap = warp_stream_cap(longest, run.S_w, min_step, run.half);
    DevBufs D;
    if (plan.on()) {
        const int Kp = resample_pitch(plan);
        std::vector<float> t((size_t)plan.L * Kp);
        resample_table(plan, t.data(), Kp);
        const float *dt = D.up(t.data(), t.size());
        for (WarpRateRow &r : run.rrows) {
            r.table = dt;
            r.Kp = Kp;
            r.K = (int32_t)plan.K;
        }
    }
    return walk_warp_pieces(run, D, x, B, S, n_cap, piece_bounds, n_pieces, y, S_w, ranges, max_ranges);
}
}  // namespace
}  // extern "C++"

int vits_test_warp_pieces(int device_id, const float *x, const int64_t *counts, int B, int S, const vits_warp_seg *segs, const int32_t *seg_first,
                          const int64_t *piece_bounds, int n_pieces, float *y, int S_w, int64_t *ranges, int max_ranges) {
    return test_warp_pieces_as(device_id, x, counts, B, S, segs, seg_first, nullptr, piece_bounds, n_pieces, y, S_w, ranges, max_ranges,
                               warp_segs_fault, &WarpRun::wsegs);
}

int vits_test_glide_pieces(int device_id, const float *x, const int64_t *counts, int B, int S, const vits_glide_seg *segs, const int32_t *seg_first,
                           const int64_t *piece_bounds, int n_pieces, float *y, int S_w, int64_t *ranges, int max_ranges) {
    return test_warp_pieces_as(device_id, x, counts, B, S, segs, seg_first, nullptr, piece_bounds, n_pieces, y, S_w, ranges, max_ranges,
                               glide_segs_fault, &WarpRun::gsegs);
}

int vits_test_warp_rate_pieces(int device_id, const float *x, const int64_t *counts, int B, int S, const vits_warp_seg *segs,
                               const int32_t *seg_first, int in_rate, int out_rate, const int64_t *piece_bounds, int n_pieces, float *y, int S_w,
                               int64_t *ranges, int max_ranges) {
    const int rates[2] = {in_rate, out_rate};
    return test_warp_pieces_as(device_id, x, counts, B, S, segs, seg_first, rates, piece_bounds, n_pieces, y, S_w, ranges, max_ranges,
                               warp_rate_segs_fault, &WarpRun::wsegs);
}

int vits_test_glide_rate_pieces(int device_id, const float *x, const int64_t *counts, int B, int S, const vits_glide_seg *segs,
                                const int32_t *seg_first, int in_rate, int out_rate, const int64_t *piece_bounds, int n_pieces, float *y, int S_w,
                                int64_t *ranges, int max_ranges) {
    const int rates[2] = {in_rate, out_rate};
    return test_warp_pieces_as(device_id, x, counts, B, S, segs, seg_first, rates, piece_bounds, n_pieces, y, S_w, ranges, max_ranges,
                               glide_rate_segs_fault, &WarpRun::gsegs);
}

// The rows entry by value: the plans of the distinct rates among out_rates (0 or in_rate: a native row), one record per row,
// one launch.  y is [B][S_out], S_out = max_b n_out[b].
int vits_test_resample_rows(int device_id, const float *x, const int64_t *lens, int B, int S, int in_rate, const int32_t *out_rates,
                            float *y, size_t y_elems, int64_t *n_out) {
    if (int rc = test_dev(device_id)) return rc;
    if (!x || !y || !lens || !out_rates || !n_out || B <= 0 || S <= 0) return fail(nullptr, VITS_E_ARG, "bad resampler test arguments");
    DevBufs D;
    std::vector<ResampleDev> plans;
    std::vector<ResampleRowPlan> recs((size_t)B);
    std::vector<int> n_in(B), no(B);
    int64_t S_out = 0;
    int lds = 0;
    for (int b = 0; b < B; b++) {
        const int fo = out_rates[b];
        if (fo < 0) return fail(nullptr, VITS_E_ARG, "row %d: output rate %d is negative", b, fo);
        const int64_t n = lens[b] < 0 ? 0 : (lens[b] > S ? S : lens[b]);
        int64_t N = n;
        if (fo != 0 && fo != in_rate) {
            size_t k = 0;
            while (k < plans.size() && plans[k].plan.fo != fo) k++;
            if (k == plans.size()) {
                if (k == VITS_MAX_ROW_RATES) return fail(nullptr, VITS_E_ARG, "row %d: more than %d distinct resampling rates", b, VITS_MAX_ROW_RATES);
                ResampleDev d;
                const std::string e = resample_plan(in_rate, fo, d.plan);
                if (!e.empty()) return fail(nullptr, VITS_E_ARG, "row %d: %s", b, e.c_str());
                d.Kp = resample_pitch(d.plan);
                std::vector<float> tab((size_t)d.plan.L * d.Kp);
                resample_table(d.plan, tab.data(), d.Kp);
                d.table = D.up(tab.data(), tab.size());
                plans.push_back(d);
            }
            recs[b] = resample_row_plan(&plans[k]);
            N = plans[k].plan.count(n);
            if (N > INT_MAX) return fail(nullptr, VITS_E_ARG, "row %d: %lld samples at %d Hz", b, (long long)N, fo);
        } else {
            recs[b] = resample_row_plan(nullptr);
        }
        lds = recs[b].span > lds ? recs[b].span : lds;
        n_in[b] = (int)n;
        no[b] = (int)N;
        n_out[b] = N;
        S_out = N > S_out ? N : S_out;
    }
    if (y_elems < (size_t)B * (size_t)S_out)
        return fail(nullptr, VITS_E_ARG, "y holds %zu elements, %d rows of %lld need %zu", y_elems, B, (long long)S_out, (size_t)B * (size_t)S_out);
    if (S_out == 0) return VITS_OK;
    float *dx = D.up(x, (size_t)B * S);
    float *dy = D.fill<float>((size_t)B * S_out, 0xff);
    ResampleRowsArgs r{};
    r.plans = D.up(recs.data(), recs.size());
    r.x = dx;
    r.x_pitch = S;
    r.x_n = S;
    r.n_in = D.up(n_in.data(), (size_t)B);
    r.n_out = D.up(no.data(), (size_t)B);
    r.y = dy;
    r.y_pitch = S_out;
    r.n_hi = (int)S_out;
    TCHECK(D.err);
    TCHECK(launch_resample_rows(r, B, lds, nullptr));
    TCHECK(hipDeviceSynchronize());
    TCHECK(download(y, dy, (size_t)B * S_out));
    return VITS_OK;
}

// A hook's side of every delivery (the sequence: delivery_run.hip.hpp, the handle's own): x uploaded, the call's buffers in one
// allocation carved by the handle's walk, nothing behind the first wait.
static int test_deliver_run(int device_id, const float *x, const int64_t *counts, int B, int S, const DeliveryRequest &rq,
                            const DeliveryOutputs &out) {
    if (!x || !counts || B <= 0 || S <= 0 || (int64_t)B * S > (int64_t)1 << 40) return fail(nullptr, VITS_E_ARG, "bad delivery test arguments");
    for (int b = 0; b < B; b++)
        if (counts[b] < 0 || counts[b] > S) return fail(nullptr, VITS_E_ARG, "counts[%d] = %lld outside [0, %d]", b, (long long)counts[b], S);
    DevBufs D;
    auto bufs = [&](const DeliveryNeeds &need, const float *&d_x, DeliveryCallBufs &cb) -> DeliveryStatus {
        if (int rc = test_dev(device_id)) return {rc, g_open_error};
        d_x = D.up(x, (size_t)B * S);
        const size_t total = carved_bytes([&](Carver &cv) { carve_delivery_call(cv, B, S, need); });
        Carver cv(D.alloc<unsigned char>(total), total);
        if (!D.ok()) return delivery_refusal(VITS_E_DEVICE, "delivery test buffers: %s", hipGetErrorString(D.err));
        cb = carve_delivery_call(cv, B, S, need);
        if (!cv.fits()) return delivery_refusal(VITS_E_NOMEM, "delivery walk carved %zu of %zu bytes", cv.used, cv.cap);
        return {};
    };
    const DeliveryStatus s = delivery_run(counts, B, S, nullptr, rq, out, bufs, [] { return DeliveryStatus{}; });
    return s.code ? fail(nullptr, s.code, "%s", s.msg.c_str()) : VITS_OK;
}

int vits_test_deliver(int device_id, const float *x, const int64_t *counts, int B, int S, const vits_segment *segs, int n_segs,
                      int n_streams, int encoding, void *dst, size_t dst_bytes, int64_t *stream_samples, int64_t *stream_offsets) {
    return test_deliver_run(device_id, x, counts, B, S,
                            {segs, nullptr, nullptr, nullptr, nullptr, 0, n_segs, n_streams, encoding, 0, dst, dst_bytes, /*kept=*/false},
                            {stream_samples, stream_offsets, nullptr, nullptr, nullptr, nullptr});
}

int vits_test_deliver_trimmed(int device_id, const float *x, const int64_t *counts, int B, int S, const vits_segment *segs,
                              const vits_trim *trims, int n_segs, int n_streams, int encoding, void *dst, size_t dst_bytes,
                              int64_t *stream_samples, int64_t *stream_offsets, int64_t *kept_first, int64_t *kept_count) {
    return test_deliver_run(device_id, x, counts, B, S,
                            {segs, trims, nullptr, nullptr, nullptr, 0, n_segs, n_streams, encoding, 0, dst, dst_bytes, /*kept=*/true},
                            {stream_samples, stream_offsets, kept_first, kept_count, nullptr, nullptr});
}

int vits_test_deliver_leveled(int device_id, const float *x, const int64_t *counts, int B, int S, const vits_segment *segs,
                              const vits_trim *trims, const vits_level *levels, int n_segs, int n_streams, int encoding,
                              int sample_rate, void *dst, size_t dst_bytes, int64_t *stream_samples, int64_t *stream_offsets,
                              int64_t *kept_first, int64_t *kept_count, double *loudness, float *gain) {
    return test_deliver_run(device_id, x, counts, B, S,
                            {segs, trims, levels, nullptr, nullptr, 0, n_segs, n_streams, encoding, sample_rate, dst, dst_bytes, /*kept=*/true},
                            {stream_samples, stream_offsets, kept_first, kept_count, loudness, gain});
}

int vits_test_deliver_shaped(int device_id, const float *x, const int64_t *counts, int B, int S, const vits_segment *segs,
                             const vits_trim *trims, const vits_level *levels, const vits_shape *shapes, const vits_env_point *points,
                             int64_t n_points, int n_segs, int n_streams, int encoding, int sample_rate, void *dst, size_t dst_bytes,
                             int64_t *stream_samples, int64_t *stream_offsets, int64_t *kept_first, int64_t *kept_count,
                             double *loudness, float *gain) {
    return test_deliver_run(device_id, x, counts, B, S,
                            {segs, trims, levels, shapes, points, n_points, n_segs, n_streams, encoding, sample_rate, dst, dst_bytes, /*kept=*/true},
                            {stream_samples, stream_offsets, kept_first, kept_count, loudness, gain});
}

int vits_test_deliver_limited(int device_id, const float *x, const int64_t *counts, int B, int S, const vits_segment *segs,
                              const vits_trim *trims, const vits_level *levels, const vits_shape *shapes, const vits_env_point *points,
                              int64_t n_points, const vits_limit *limits, int n_segs, int n_streams, int encoding, int sample_rate,
                              void *dst, size_t dst_bytes, int64_t *stream_samples, int64_t *stream_offsets, int64_t *kept_first,
                              int64_t *kept_count, double *loudness, float *gain) {
    return test_deliver_run(device_id, x, counts, B, S,
                            {segs, trims, levels, shapes, points, n_points, n_segs, n_streams, encoding, sample_rate, dst, dst_bytes, /*kept=*/true, limits},
                            {stream_samples, stream_offsets, kept_first, kept_count, loudness, gain});
}

int vits_test_loudness_blocks(int device_id, const float *x, const int64_t *counts, const int64_t *firsts, int B, int S,
                              int sample_rate, float *e, size_t e_cap, int32_t *n_sub, int32_t *chunk) {
    if (chunk) *chunk = kLoudChunk;
    if (!x || !counts || !firsts || !n_sub || B <= 0 || S <= 0 || (int64_t)B * S > (int64_t)1 << 40)
        return fail(nullptr, VITS_E_ARG, "bad loudness test arguments");
    if (sample_rate < kLevelMinRate || sample_rate > kLevelMaxRate)
        return fail(nullptr, VITS_E_ARG, "sample_rate %d outside [%d, %d]", sample_rate, kLevelMinRate, kLevelMaxRate);
    const LoudCoef k = loudness_coef(sample_rate);
    std::vector<LoudSeg> ls(B);
    int64_t chunks = 0, subs = 0;
    int max_n = 0;
    for (int b = 0; b < B; b++) {
        if (firsts[b] < 0 || counts[b] < 0 || firsts[b] + counts[b] > S)
            return fail(nullptr, VITS_E_ARG, "row %d: kept range [%lld, +%lld) outside [0, %d]", b, (long long)firsts[b], (long long)counts[b], S);
        n_sub[b] = (int32_t)(counts[b] / k.hop);
        ls[b] = LoudSeg{(int64_t)b * S + firsts[b], chunks, subs, n_sub[b] * k.hop, 0};
        chunks += ((int64_t)ls[b].n + kLoudChunk - 1) / kLoudChunk;
        subs += n_sub[b];
        max_n = ls[b].n > max_n ? ls[b].n : max_n;
    }
    if ((size_t)subs > e_cap || (subs > 0 && !e)) return fail(nullptr, VITS_E_ARG, "energy buffer too small: %zu < %lld", e_cap, (long long)subs);
    if (int rc = test_dev(device_id)) return rc;
    DevBufs D;
    float *dx = D.up(x, (size_t)B * S);
    // the pipeline's buffers, by the pipeline's walk
    const size_t total = carved_bytes([&](Carver &cv) { carve_level(cv, B, S); });
    Carver cv(D.alloc<unsigned char>(total), total);
    TCHECK(D.err);
    const LevelBufs lb = carve_level(cv, B, S);
    if (max_n > 0) {
        TCHECK(hipMemcpy(lb.segs, ls.data(), ls.size() * sizeof(LoudSeg), hipMemcpyHostToDevice));
        const hipError_t enq = launch_loudness(dx, lb.segs, B, max_n, k, lb.fin, lb.init, lb.part, lb.e(), nullptr);
        const hipError_t done = hipDeviceSynchronize();
        TCHECK(enq);
        TCHECK(done);
        TCHECK(download(e, lb.e(), (size_t)subs));
    }
    return VITS_OK;
}

// The encoded stream's pieces by value: what both hooks are.  x [B][S] in pieces of piece_samples through the pipeline's pack
// stage (stream_run.hip.hpp) over the pipeline's walk - `shaped`: through the shaped stream's kernels, with `shaping`
// (nullable) - and every piece's bytes and peaks out in one copy, as the pipeline.  firsts / ns: nullable.
namespace {
int stream_pack_test(int device_id, const float *x, const int64_t *counts, int B, int S, int piece_samples, const vits_stream_format *fmt,
                     bool shaped, const vits_stream_shaping *shaping, void *bytes, size_t bytes_cap, int64_t *pitches, int32_t *valid,
                     float *peaks, int64_t *firsts, int64_t *ns, int max_pieces, const vits_stream_onset *onsets = nullptr,
                     int32_t *skip = nullptr, int32_t *start_out = nullptr) {
    if (!x || !counts || !bytes || !pitches || !valid || !peaks || B <= 0 || B > 65535 || S <= 0 || piece_samples < 1 ||
        (int64_t)B * S > (int64_t)1 << 40)
        return fail(nullptr, VITS_E_ARG, "bad stream pack test arguments");
    for (int b = 0; b < B; b++)
        if (counts[b] < 0 || counts[b] > S) return fail(nullptr, VITS_E_ARG, "counts[%d] = %lld outside [0, %d]", b, (long long)counts[b], S);
    if (int rc = host_stream_format(nullptr, fmt, B)) return rc;
    if (shaped)
        if (int rc = host_stream_shaping(nullptr, shaping, fmt, B)) return rc;
    if (int rc = host_stream_onsets(nullptr, onsets, fmt, B)) return rc;
    const bool trimmed = stream_trimmed(onsets, B);
    const vits_stream_shaping none{};
    const vits_stream_shaping *shp = !shaped ? nullptr : (shaping ? shaping : &none);  // (the shaped hook always runs the shaped kernels)
    const int L = shp ? shp->lookahead : 0;
    const int w = delivery_width(fmt->encoding);
    const int64_t pieces = ((int64_t)S + piece_samples - 1) / piece_samples;
    size_t need = 0;
    for (int64_t f0 = 0; f0 < S; f0 += piece_samples) {
        int64_t ef, en;
        stream_emit_range(f0, S - f0 > piece_samples ? piece_samples : S - f0, f0 + piece_samples >= S, S, L, ef, en);
        if (en > 0) need += (size_t)B * StreamPackBufs::pitch(w, en);
    }
    if (pieces > max_pieces || need > bytes_cap)
        return fail(nullptr, VITS_E_ARG, "%lld pieces of %zu bytes: room for %d pieces and %zu bytes", (long long)pieces, need, max_pieces, bytes_cap);
    if (int rc = test_dev(device_id)) return rc;
    DevBufs D;
    float *dx = D.up(x, (size_t)B * S);
    std::vector<int> c32((size_t)B);
    for (int b = 0; b < B; b++) c32[b] = (int)counts[b];
    int *dcount = D.up(c32.data(), (size_t)B);
    // the pipeline's buffers, by the pipeline's walk
    const int64_t n_max = stream_n_max(ResamplePlan{}, piece_samples, S, 1, L, S);  // (piece_samples "frames" of one sample)
    const auto walk = [&](Carver &cv) {
        return carve_stream(cv, B, S, n_max, 0, /*enc=*/true, shaped, L, shaped ? stream_knot_count(shp, B) : 0, trimmed);
    };
    const size_t total = carved_bytes(walk);
    Carver cv(D.alloc<unsigned char>(total), total);
    TCHECK(D.err);
    const StreamBufs sb = walk(cv);
    if (!cv.fits()) return fail(nullptr, VITS_E_NOMEM, "stream walk carved %zu of %zu bytes", cv.used, cv.cap);
    StreamPackRun run;
    TCHECK(stream_pack_begin(run, fmt, shp, B, sb.sp, sb.ss, StreamPackRows{dcount, 1, S}, S, nullptr, trimmed ? onsets : nullptr, counts));
    unsigned char *dst = static_cast<unsigned char *>(bytes);
    std::vector<unsigned char> landing;
    std::vector<int32_t> start((size_t)B, 0);
    int k = 0;
    for (int64_t f0 = 0; f0 < S; f0 += piece_samples, k++) {
        int64_t ef = 0, en = 0;
        unsigned char *d = nullptr;
        size_t pitch = 0;
        int launches = 0;
        const int64_t n = S - f0 > piece_samples ? piece_samples : S - f0;
        const hipError_t enq = stream_pack_piece(run, dx + f0, S, f0, n, B, nullptr, d, ef, en, pitch, launches);
        const hipError_t done = hipDeviceSynchronize();
        TCHECK(enq);
        TCHECK(done);
        if (firsts) firsts[k] = ef;
        if (ns) ns[k] = en;
        pitches[k] = 0;
        if (en <= 0) continue;
        landing.resize((size_t)B * pitch + run.tail_bytes(B));
        TCHECK(hipMemcpy(landing.data(), d, landing.size(), hipMemcpyDeviceToHost));  // bytes, peaks (and starts) in one copy, as the pipeline
        std::memcpy(dst, landing.data(), (size_t)B * pitch);
        std::memcpy(peaks + (size_t)k * B, landing.data() + (size_t)B * pitch, (size_t)B * sizeof(float));
        dst += (size_t)B * pitch;
        pitches[k] = (int64_t)pitch;
        for (int b = 0; b < B; b++) valid[(size_t)k * B + b] = (int32_t)std::clamp<int64_t>(counts[b] - ef, 0, en);
        if (trimmed) {
            std::memcpy(start.data(), landing.data() + (size_t)B * pitch + StreamPackBufs::peak_floats(B) * sizeof(float), (size_t)B * sizeof(int32_t));
            stream_pack_seen(run, start.data(), ef + en, B);
        }
        for (int b = 0; b < B && skip; b++)
            skip[(size_t)k * B + b] = (int32_t)std::clamp<int64_t>((int64_t)start[b] - ef, 0, valid[(size_t)k * B + b]);
    }
    for (int b = 0; b < B && start_out; b++) start_out[b] = start[b];
    return k;
}
}  // namespace

int vits_test_stream_pack(int device_id, const float *x, const int64_t *counts, int B, int S, int piece_samples,
                          const vits_stream_format *fmt, void *bytes, size_t bytes_cap, int64_t *pitches, int32_t *valid, float *peaks,
                          int max_pieces) {
    return stream_pack_test(device_id, x, counts, B, S, piece_samples, fmt, /*shaped=*/false, nullptr, bytes, bytes_cap, pitches, valid, peaks,
                            nullptr, nullptr, max_pieces);
}

int vits_test_stream_pack_shaped(int device_id, const float *x, const int64_t *counts, int B, int S, int piece_samples,
                                 const vits_stream_format *fmt, const vits_stream_shaping *shaping, void *bytes, size_t bytes_cap,
                                 int64_t *pitches, int32_t *valid, float *peaks, int64_t *firsts, int64_t *ns, int max_pieces) {
    if (!firsts || !ns) return fail(nullptr, VITS_E_ARG, "bad stream pack test arguments");
    return stream_pack_test(device_id, x, counts, B, S, piece_samples, fmt, /*shaped=*/true, shaping, bytes, bytes_cap, pitches, valid, peaks,
                            firsts, ns, max_pieces);
}

int vits_test_stream_pack_trimmed(int device_id, const float *x, const int64_t *counts, int B, int S, int piece_samples,
                                  const vits_stream_format *fmt, const vits_stream_shaping *shaping, const vits_stream_onset *onsets, void *bytes,
                                  size_t bytes_cap, int64_t *pitches, int32_t *valid, int32_t *skip, float *peaks, int64_t *firsts, int64_t *ns,
                                  int32_t *start, int max_pieces) {
    if (!firsts || !ns || !skip || !start) return fail(nullptr, VITS_E_ARG, "bad stream pack test arguments");
    return stream_pack_test(device_id, x, counts, B, S, piece_samples, fmt, /*shaped=*/true, shaping, bytes, bytes_cap, pitches, valid, peaks,
                            firsts, ns, max_pieces, onsets, skip, start);
}

int vits_test_resample_pieces(int device_id, const float *x, const int64_t *lens, int B, int S, int in_rate, int out_rate,
                              int piece_samples, float *y, int64_t S_out, int64_t *ranges, int max_ranges) {
    if (int rc = test_dev(device_id)) return rc;
    if (!x || !y || piece_samples < 1) return fail(nullptr, VITS_E_ARG, "bad resampler test arguments");
    DevBufs D;
    ResampleTest t;
    if (int rc = resample_test_setup(D, lens, B, S, in_rate, out_rate, t)) return rc;
    const ResamplePlan &p = t.dev.plan;
    const int total = (int)p.count(S);
    if (S_out < total) return fail(nullptr, VITS_E_ARG, "S_out = %lld, %d input samples give %d", (long long)S_out, S, total);
    float *dx = D.up(x, (size_t)B * S);
    // the pipeline's buffers, by the pipeline's walk (poisoned); the rows' counts by its kernel, from the clipped lens
    const auto walk = [&](Carver &cv) { return carve_stream(cv, B, total, total, (int)p.K, /*enc=*/false, false, 0, 0); };
    const size_t bytes = carved_bytes(walk);
    Carver cv(D.fill<unsigned char>(bytes, 0xff), bytes);
    TCHECK(D.err);
    const StreamBufs sb = walk(cv);
    if (!cv.fits()) return fail(nullptr, VITS_E_NOMEM, "stream walk carved %zu of %zu bytes", cv.used, cv.cap);
    ResampleRun run;
    TCHECK(resample_run_begin(run, t.dev, sb.rs, t.d_n_in, 1, S, total, B, nullptr));
    std::vector<float> piece((size_t)B * total);
    std::memset(y, 0, (size_t)B * S_out * sizeof(float));
    int calls = 0;
    for (int64_t f0 = 0; f0 < S; f0 += piece_samples) {
        const int64_t n = S - f0 > piece_samples ? piece_samples : S - f0;
        int64_t ef = 0, en = 0;
        int launches = 0;
        TCHECK(resample_run_piece(run, dx + f0, S, f0, n, f0 + n == S, B, nullptr, ef, en, launches));
        if (en <= 0) continue;  // (a piece shorter than the filter's look-ahead completes nothing)
        TCHECK(hipDeviceSynchronize());
        TCHECK(download(piece.data(), sb.rs.out, (size_t)B * en));
        for (int b = 0; b < B; b++) std::memcpy(y + (size_t)b * S_out + ef, piece.data() + (size_t)b * en, (size_t)en * sizeof(float));
        if (ranges && calls < max_ranges) {
            ranges[2 * calls] = ef;
            ranges[2 * calls + 1] = en;
        }
        calls++;
    }
    TCHECK(hipDeviceSynchronize());
    return calls;
}

// The token-to-frame and frame-to-sample kernels by value.  Each hook checks on the host whatever a kernel could read or
// write out of bounds with, then launches through the pipeline's own launch_* function.
namespace {
// lens [B] within [0, T], as int for the kernels
int glue_test_lens(const int64_t *lens, int B, int T, std::vector<int> &l32) {
    if (!lens || B <= 0 || B > 65535 || T <= 0) return fail(nullptr, VITS_E_ARG, "bad sizes (B=%d, T=%d) or null lens", B, T);
    l32.resize(B);
    for (int b = 0; b < B; b++) {
        if (lens[b] < 0 || lens[b] > T) return fail(nullptr, VITS_E_ARG, "lens[%d]=%lld outside [0,%d]", b, (long long)lens[b], T);
        l32[b] = (int)lens[b];
    }
    return VITS_OK;
}
}  // namespace

int vits_test_durations(int device_id, const float *logw, const int64_t *dur, const int64_t *lens, int B, int T, float length_scale,
                        const float *rows, const float *token_rate, float *w_ceil, int32_t *cum, int32_t *y_len) {
    if (int rc = test_dev(device_id)) return rc;
    std::vector<int> l32;
    if (int rc = glue_test_lens(lens, B, T, l32)) return rc;
    if (!w_ceil || !cum || !y_len || (logw != nullptr) == (dur != nullptr))
        return fail(nullptr, VITS_E_ARG, "one of logw and dur, and three outputs, are needed");
    if (dur && token_rate) return fail(nullptr, VITS_E_ARG, "forced durations leave nothing to scale");
    if (dur)
        for (int b = 0; b < B; b++) {
            int64_t sum = 0;
            for (int t = 0; t < l32[b]; t++) {
                const int64_t d = dur[(size_t)b * T + t];
                if (d < 0 || d > VITS_MAX_FORCED_FRAMES || (sum += d) > VITS_MAX_FORCED_FRAMES)
                    return fail(nullptr, VITS_E_ARG, "dur[%d,%d]=%lld is negative or passes %d frames in its row", b, t, (long long)d,
                                VITS_MAX_FORCED_FRAMES);
            }
        }
    const size_t nBT = (size_t)B * T;
    DevBufs D;
    int *dlen = D.up(l32.data(), (size_t)B);
    const float *drows = rows ? D.up(rows, (size_t)B * 3) : nullptr;
    float *dw = D.fill<float>(nBT, 0xff);
    int *dcum = D.fill<int>(nBT, 0xff), *dyl = D.fill<int>((size_t)B, 0xff);
    if (dur) {
        const int64_t *dd = D.up(dur, nBT);
        TCHECK(D.err);
        launch_forced_durations(nullptr, B, T, dd, dlen, dw, dcum, dyl);
    } else {
        const float *dl = D.up(logw, nBT);
        const float *dr = token_rate ? D.up(token_rate, nBT) : nullptr;
        TCHECK(D.err);
        launch_durations(nullptr, B, T, dl, dlen, length_scale, drows, dr, dw, dcum, dyl);
    }
    TCHECK(hipGetLastError());
    TCHECK(hipDeviceSynchronize());
    TCHECK(download(w_ceil, dw, nBT));
    TCHECK(download(cum, dcum, nBT));
    TCHECK(download(y_len, dyl, (size_t)B));
    return VITS_OK;
}

int vits_test_fit_durations(int device_id, const float *w, const int64_t *lens, int B, int T, const vits_fit *fit, float *w_ceil,
                            int32_t *cum, int32_t *y_len, double *scale, int64_t *frames, int32_t *status) {
    if (int rc = test_dev(device_id)) return rc;
    std::vector<int> l32;
    if (int rc = glue_test_lens(lens, B, T, l32)) return rc;
    if (!w || !fit || !w_ceil || !cum || !y_len) return fail(nullptr, VITS_E_ARG, "weights, a fit and three outputs are needed");
    const std::string e = fit_fault(fit, B, VITS_MAX_FORCED_FRAMES);
    if (!e.empty()) return fail(nullptr, VITS_E_ARG, "%s", e.c_str());
    const int G = fit->n_groups;
    if (G < 1) return fail(nullptr, VITS_E_ARG, "fit n_groups = %d: nothing to launch", G);
    const size_t nBT = (size_t)B * T;
    std::vector<int> g32(fit->group, fit->group + B), m32(fit->mode, fit->mode + G);
    std::vector<FitResult> res((size_t)G);
    DevBufs D;
    const float *dwt = D.up(w, nBT);
    int *dlen = D.up(l32.data(), (size_t)B), *dg = D.up(g32.data(), (size_t)B), *dm = D.up(m32.data(), (size_t)G);
    int64_t *dt = D.up(fit->target_frames, (size_t)G);
    float *dw = D.up(w_ceil, nBT);
    int *dcum = D.up(cum, nBT), *dyl = D.up(y_len, (size_t)B);
    FitResult *dres = D.fill<FitResult>((size_t)G, 0xff);
    TCHECK(D.err);
    launch_fit_durations(nullptr, B, T, G, dwt, dlen, dg, dt, dm, dw, dcum, dyl, dres);
    TCHECK(hipGetLastError());
    TCHECK(hipDeviceSynchronize());
    TCHECK(download(w_ceil, dw, nBT));
    TCHECK(download(cum, dcum, nBT));
    TCHECK(download(y_len, dyl, (size_t)B));
    TCHECK(download(res.data(), dres, (size_t)G));
    for (int g = 0; g < G; g++) {
        if (scale) scale[g] = res[g].scale;
        if (frames) frames[g] = res[g].frames;
        if (status) status[g] = res[g].status;
    }
    return VITS_OK;
}

int vits_test_expand_prior(int device_id, const float *m_logs, int B, int C, int T, const int32_t *cum, const int64_t *lens,
                           const int32_t *y_len, int F, const float *noise, int64_t noise_stride, int noise_frames,
                           float noise_scale, const float *rows, const uint64_t *seeds, float *z_p) {
    if (int rc = test_dev(device_id)) return rc;
    std::vector<int> l32;
    if (int rc = glue_test_lens(lens, B, T, l32)) return rc;
    if (!m_logs || !cum || !y_len || !z_p || C <= 0 || (C + 3) / 4 > 65535 || F <= 0)
        return fail(nullptr, VITS_E_ARG, "bad length-regulator test arguments (C=%d, F=%d)", C, F);
    if (noise && (noise_frames < 0 || noise_stride < noise_frames))
        return fail(nullptr, VITS_E_ARG, "noise_frames = %d, the noise rows hold %lld", noise_frames, (long long)noise_stride);
    for (int b = 0; b < B; b++) {
        const int32_t *cb = cum + (size_t)b * T;
        for (int t = 0; t < T; t++)
            if (cb[t] < (t ? cb[t - 1] : 0)) return fail(nullptr, VITS_E_ARG, "cum[%d,%d]=%d: not a running sum of frame counts", b, t, cb[t]);
        if (y_len[b] != (cb[T - 1] < 1 ? 1 : cb[T - 1]) || y_len[b] > F)
            return fail(nullptr, VITS_E_ARG, "y_len[%d]=%d with cum ending at %d and F=%d", b, y_len[b], cb[T - 1], F);
    }
    const size_t nBT = (size_t)B * T, nz = (size_t)B * C * F;
    DevBufs D;
    const float *dm = D.up(m_logs, nBT * 2 * C);
    const int *dcum = D.up(cum, nBT), *dlen = D.up(l32.data(), (size_t)B), *dyl = D.up(y_len, (size_t)B);
    const float *dn = noise ? D.up(noise, (size_t)B * C * noise_stride) : nullptr;
    const float *drows = rows ? D.up(rows, (size_t)B * 3) : nullptr;
    const uint64_t *dseeds = !noise && seeds ? D.up(seeds, (size_t)B) : nullptr;
    float *dz = D.fill<float>(nz, 0xff);
    TCHECK(D.err);
    launch_expand_prior(nullptr, B, C, T, F, dm, dm + (size_t)C * T, (int64_t)2 * C * T, dcum, dlen, dyl, dn, noise_stride, noise_scale,
                        drows, dseeds, dz, noise ? noise_frames : F);
    TCHECK(hipGetLastError());
    TCHECK(hipDeviceSynchronize());
    TCHECK(download(z_p, dz, nz));
    return VITS_OK;
}

int vits_test_fill_normal(int device_id, int64_t n, uint64_t seed, uint64_t stream_id, float *out) {
    if (int rc = test_dev(device_id)) return rc;
    if (!out || n < 0 || n > ((int64_t)1 << 28)) return fail(nullptr, VITS_E_ARG, "n = %lld outside [0, 2^28] or null output", (long long)n);
    DevBufs D;
    float *d = D.fill<float>((size_t)n, 0xff);
    TCHECK(D.err);
    launch_fill_normal(nullptr, d, n, seed, stream_id);
    TCHECK(hipGetLastError());
    TCHECK(hipDeviceSynchronize());
    TCHECK(download(out, d, (size_t)n));
    return VITS_OK;
}

int vits_test_fill_normal_rows(int device_id, int B, int channels, int T, const uint64_t *seeds, uint32_t stream, const float *rows,
                               int col, float *out) {
    if (int rc = test_dev(device_id)) return rc;
    if (!seeds || !rows || !out || B <= 0 || B > 65535 || channels <= 0 || channels > 65535 || T <= 0 || col < 0 || col > 2)
        return fail(nullptr, VITS_E_ARG, "bad row-noise test arguments (B=%d, channels=%d, T=%d, col=%d)", B, channels, T, col);
    const size_t n = (size_t)B * channels * T;
    DevBufs D;
    const uint64_t *ds = D.up(seeds, (size_t)B);
    const float *dr = D.up(rows, (size_t)B * 3);
    float *d = D.fill<float>(n, 0xff);
    TCHECK(D.err);
    launch_fill_normal_rows(nullptr, B, channels, T, d, ds, stream, dr, col);
    TCHECK(hipGetLastError());
    TCHECK(hipDeviceSynchronize());
    TCHECK(download(out, d, n));
    return VITS_OK;
}

int vits_test_post_conv(int device_id, const float *x, int B, int C, int T, const float *w, int K, float slope, const int64_t *vlen,
                        int hop, int kernel, float *out) {
    if (int rc = test_dev(device_id)) return rc;
    if (!x || !w || !out || B <= 0 || B > 65535 || C <= 0 || T <= 0 || K <= 0 || K > 4096 || hop < 1 || kernel < 0 || kernel > 2)
        return fail(nullptr, VITS_E_ARG, "bad vocoder-tail test arguments (B=%d, C=%d, T=%d, K=%d, hop=%d, kernel=%d)", B, C, T, K, hop, kernel);
    if (kernel != 0 && C % 8) return fail(nullptr, VITS_E_ARG, "the blocked layout holds 8 channels per cell: C=%d", C);
    const size_t lds = kernel == 0 ? post_conv_lds(C, K) : post_conv_blocked_lds(C, K);
    if (lds > 64 * 1024) return fail(nullptr, VITS_E_ARG, "C=%d, K=%d need %zu bytes of LDS: more than 64 KiB", C, K, lds);
    std::vector<int> v32;
    if (vlen)
        for (int b = 0; b < B; b++) {
            if (vlen[b] < 0 || vlen[b] > INT_MAX) return fail(nullptr, VITS_E_ARG, "vlen[%d]=%lld is not a frame count", b, (long long)vlen[b]);
            v32.push_back((int)vlen[b]);
        }
    const size_t nx = (size_t)B * C * T, no = (size_t)B * T;
    DevBufs D;
    const float *dx = D.up(x, nx);
    const float *dw = D.up(w, (size_t)C * K);
    const int *dv = vlen ? D.up(v32.data(), (size_t)B) : nullptr;
    float *dout = D.fill<float>(no, 0xff);
    TCHECK(D.err);
    if (kernel == 0) launch_post_conv(nullptr, B, C, K, T, dx, dw, dout, slope, dv, hop);
    else launch_post_conv_blocked(nullptr, B, C, K, T, dx, dw, dout, slope, dv, hop, kernel == 2);
    TCHECK(hipGetLastError());
    TCHECK(hipDeviceSynchronize());
    TCHECK(download(out, dout, no));
    return VITS_OK;
}

// The text-side kernels of the encoder and the stochastic duration predictor by value (launch_layernorm ... launch_ea_logw
// above).  Every output is pre-filled with 0xff bytes (NaN as fp32 and as fp16) and downloaded together with a guard row of T
// elements (T cells of 8 for planes) behind it, so the caller sees an element never written and a write past the tensor's end.
namespace {
int sdp_test_sizes(const char *what, int B, int C, int T) {
    if (B <= 0 || B > 65535 || C <= 0 || C > 65535 || T <= 0 || (int64_t)B * C * T > ((int64_t)1 << 28))
        return fail(nullptr, VITS_E_ARG, "%s: bad sizes (B=%d, C=%d, T=%d)", what, B, C, T);
    return VITS_OK;
}
// `n` elements of `host` in front of a 0xff guard of `guard` elements
float *up_guarded(DevBufs &D, const float *host, size_t n, size_t guard) {
    float *d = D.fill<float>(n + guard, 0xff);
    if (d && host && n && D.ok()) D.err = hipMemcpy(d, host, n * sizeof(float), hipMemcpyHostToDevice);
    return d;
}
}  // namespace

int vits_test_layernorm(int device_id, const float *x, const float *out_init, int B, int C, int T, const float *gamma,
                        const float *beta, const int64_t *lens, int flags, int form, int in_place, const float *dw_w,
                        const float *dw_b, int K, int dil, float *out, uint16_t *planes) {
    if (int rc = test_dev(device_id)) return rc;
    if (int rc = sdp_test_sizes("layernorm", B, C, T)) return rc;
    if (!x || !gamma || !beta || !out || flags < 0 || flags > 15 || form < LN_FORM_TILE16 || form > LN_FORM_COLUMN)
        return fail(nullptr, VITS_E_ARG, "layernorm: null tensor, flags=%d or form=%d", flags, form);
    std::vector<int> l32;
    if (lens)
        if (int rc = glue_test_lens(lens, B, T, l32)) return rc;
    if (!lens && ((flags & LN_MASK) || dw_w)) return fail(nullptr, VITS_E_ARG, "layernorm: LN_MASK and the depthwise conv need lens");
    if (form != LN_FORM_COLUMN && C > 256) return fail(nullptr, VITS_E_ARG, "layernorm: the tile forms hold C <= 256 (C=%d)", C);
    if (in_place && out_init) return fail(nullptr, VITS_E_ARG, "layernorm: in place, x is the initial content of out");
    if (dw_w) {  // (the pipeline forms depthwise + LN + GELU out of place, by width, without planes: launch_dw_ln)
        if (!dw_b || K < 1 || K > 15 || dil < 1 || dil > 65536 || in_place || planes || flags != LN_GELU || form == LN_FORM_TILE16 ||
            (form == LN_FORM_COLUMN) != (C > 256))
            return fail(nullptr, VITS_E_ARG, "layernorm: depthwise (K=%d, dil=%d) runs out of place, without planes, with LN_GELU alone, "
                                             "on tile32 (C <= 256) or column (C > 256)", K, dil);
    }
    if (planes && (form == LN_FORM_COLUMN || C % 8)) return fail(nullptr, VITS_E_ARG, "layernorm: planes need a tile form and C %% 8 == 0 (C=%d)", C);
    const size_t n = (size_t)B * C * T;
    DevBufs D;
    const int *dlen = lens ? D.up(l32.data(), (size_t)B) : nullptr;
    const float *dg = D.up(gamma, (size_t)C), *db = D.up(beta, (size_t)C);
    float *dout = up_guarded(D, in_place ? x : out_init, n, (size_t)T);
    const float *dx = in_place ? dout : D.up(x, n);
    uint16_t *dpl = planes ? D.fill<uint16_t>(n * 3 + (size_t)T * 8, 0xff) : nullptr;
    unsigned *dpk = planes ? D.fill<unsigned>((size_t)kSxPeakSlots * kSxPeakStride) : nullptr;
    const float *dww = dw_w ? D.up(dw_w, (size_t)C * K) : nullptr, *dwb = dw_w ? D.up(dw_b, (size_t)C) : nullptr;
    TCHECK(D.err);
    if (dw_w) launch_dw_ln(nullptr, B, C, T, K, dil, dx, dout, dww, dwb, dg, db, dlen);
    else launch_layernorm(nullptr, form, B, C, T, dx, dout, dg, db, dlen, flags, dpl, dpk);
    TCHECK(hipGetLastError());
    TCHECK(hipDeviceSynchronize());
    TCHECK(download(out, dout, n + T));
    if (planes) TCHECK(download(planes, dpl, n * 3 + (size_t)T * 8));
    return VITS_OK;
}

int vits_test_dds(int device_id, int form, const float *x, int B, int C, int T, const int64_t *lens, int n_layers,
                  const vits_test_dds_layer *layers, int mask_out, const float *head_cond, const float *head_z, int head_ch,
                  const float *head_w, const float *head_b, const float *tail_w, const float *tail_b, int tail_rows, float *out) {
    if (int rc = test_dev(device_id)) return rc;
    if (int rc = sdp_test_sizes("dds", B, C, T)) return rc;
    std::vector<int> l32;
    if (int rc = glue_test_lens(lens, B, T, l32)) return rc;
    const int nblk = C / 32;
    const bool layer16 = form == 16, head = head_cond != nullptr, tail = tail_w != nullptr;
    if ((form != 16 && form != 32) || C % 32 || C > 256 || nblk == 5 || nblk == 7 || (layer16 && (nblk & 1)))
        return fail(nullptr, VITS_E_ARG, "dds: form %d has no instantiation for C=%d", form, C);
    if (!layers || !out || n_layers < 1 || n_layers > 4 || (!head && !x))
        return fail(nullptr, VITS_E_ARG, "dds: null tensor or n_layers=%d outside [1, 4]", n_layers);
    if (!mask_out && (n_layers != 1 || head || tail))
        return fail(nullptr, VITS_E_ARG, "dds: mask_out = 0 is a single layer without head or tail (the stack masks behind its last layer)");
    if ((head || tail) && !layer16) return fail(nullptr, VITS_E_ARG, "dds: head and tail belong to the 16-column form");
    if (head && (!head_z || !head_w || !head_b || (head_ch != 0 && head_ch != 1) || n_layers < 2))
        return fail(nullptr, VITS_E_ARG, "dds: the head needs z, pre_w, pre_b, a channel 0 / 1 and a stack of >= 2 layers");
    if (tail && (tail_rows < 1 || tail_rows > C)) return fail(nullptr, VITS_E_ARG, "dds: tail rows %d outside [1, C=%d]", tail_rows, C);
    const float *pw_w[4], *pw_b[4];
    for (int l = 0; l < n_layers; l++) {
        const vits_test_dds_layer &L = layers[l];
        if (!L.dw_w || !L.dw_b || !L.ln1_g || !L.ln1_b || !L.pw_w || !L.pw_b || !L.ln2_g || !L.ln2_b || L.dil < 1 || L.dil > 65536)
            return fail(nullptr, VITS_E_ARG, "dds: layer %d has a null tensor or dil=%d", l, L.dil);
        pw_w[l] = L.pw_w;
        pw_b[l] = L.pw_b;
    }
    TestDds td;
    std::vector<float> arena;
    const std::string e = pack_test_dds(C, n_layers, pw_w, pw_b, tail_w, tail_rows, &td, &arena);
    if (!e.empty()) return fail(nullptr, VITS_E_ARG, "%s", e.c_str());
    const size_t n = (size_t)B * C * T, nc = (size_t)C;
    DevBufs D;
    const float *dA = D.up(arena.data(), arena.size());
    const int *dlen = D.up(l32.data(), (size_t)B);
    float *hbuf = up_guarded(D, head ? nullptr : x, n, (size_t)T);  // (with a head the stack never reads hbuf)
    float *y = D.fill<float>(n, 0xff), *y2 = D.fill<float>(n, 0xff);
    DdsLayerPtrs lp[4];
    for (int l = 0; l < n_layers; l++) {
        const vits_test_dds_layer &L = layers[l];
        const ConvDesc &pw = td.pw[l];
        lp[l] = {D.up(L.dw_w, nc * 3), D.up(L.dw_b, nc), D.up(L.ln1_g, nc), D.up(L.ln1_b, nc), D.up(L.ln2_g, nc), D.up(L.ln2_b, nc),
                 D.up(L.pw_b, nc), dA ? dA + td.pw16[l] : nullptr, dA ? dA + pw.w_off : nullptr, pw.CK, pw.nchunks, dds_pw_blocks(pw),
                 L.dil};
    }
    DdsHead hd{};
    if (head) hd = {D.up(head_cond, n), nullptr, D.up(head_w, nc), D.up(head_b, nc)};
    const float *dz = head ? D.up(head_z, (size_t)B * 2 * T) : nullptr;
    if (head && dz) hd.z = dz + (size_t)head_ch * T;
    DdsTail tl{};
    const size_t nt = (size_t)B * (tail ? tail_rows : 0) * T;
    if (tail) tl = {dA ? dA + td.tail16 : nullptr, tail_b ? D.up(tail_b, (size_t)tail_rows) : nullptr, D.fill<float>(nt + T, 0xff), tail_rows};
    TCHECK(D.err);
    if (mask_out) {
        TCHECK(launch_dds_stack(nullptr, layer16, B, C, T, n_layers, lp, hbuf, y, y2, dlen, head ? &hd : nullptr, tail ? &tl : nullptr));
    } else {  // one layer, launched directly: x -> y, then into the guarded buffer
        const DdsLayerPtrs &L = lp[0];
        if (layer16) {
            DdsLayer16Args q{};
            q.in = hbuf; q.out = y; q.len = dlen;
            q.dw_w = L.dw_w; q.dw_b = L.dw_b; q.ln1_g = L.ln1_g; q.ln1_b = L.ln1_b; q.ln2_g = L.ln2_g; q.ln2_b = L.ln2_b;
            q.pw16 = L.pw16; q.pw_bias = L.pw_bias; q.T = T; q.dil = L.dil; q.mask_out = 0;
            launch_dds_layer16(nullptr, B, nblk, q);
        } else {
            DdsLayerArgs a{};
            a.in = hbuf; a.out = y; a.len = dlen;
            a.dw_w = L.dw_w; a.dw_b = L.dw_b; a.ln1_g = L.ln1_g; a.ln1_b = L.ln1_b; a.ln2_g = L.ln2_g; a.ln2_b = L.ln2_b;
            a.pw = L.pw; a.pw_bias = L.pw_bias; a.C = C; a.T = T; a.dil = L.dil; a.mask_out = 0;
            a.CK = L.CK; a.nchunks = L.nchunks; a.MB = L.MB;
            launch_dds_layer32(nullptr, B, nblk, a);
        }
        TCHECK(hipGetLastError());
        TCHECK(hipMemcpyAsync(hbuf, y, n * sizeof(float), hipMemcpyDeviceToDevice, nullptr));
    }
    TCHECK(hipGetLastError());
    TCHECK(hipDeviceSynchronize());
    if (tail) TCHECK(download(out, tl.out, nt + T));
    else TCHECK(download(out, hbuf, n + T));
    return VITS_OK;
}

int vits_test_cf_pre(int device_id, const float *z, int ch, const float *w, const float *bias, const float *cond, int B, int C, int T,
                     float *out) {
    if (int rc = test_dev(device_id)) return rc;
    if (int rc = sdp_test_sizes("cf_pre", B, C, T)) return rc;
    if (!z || !w || !bias || !cond || !out || (ch != 0 && ch != 1)) return fail(nullptr, VITS_E_ARG, "cf_pre: null tensor or channel %d", ch);
    const size_t n = (size_t)B * C * T;
    DevBufs D;
    const float *dz = D.up(z, (size_t)B * 2 * T), *dw = D.up(w, (size_t)C), *db = D.up(bias, (size_t)C), *dc = D.up(cond, n);
    float *dout = D.fill<float>(n + T, 0xff);
    TCHECK(D.err);
    launch_cf_pre(nullptr, B, C, T, dz, ch, dw, db, dc, dout);
    TCHECK(hipGetLastError());
    TCHECK(hipDeviceSynchronize());
    TCHECK(download(out, dout, n + T));
    return VITS_OK;
}

int vits_test_rqs_inverse(int device_id, const float *pr, const float *z, int B, int T, const int64_t *lens, int ch0, int nb,
                          float sqrt_c, float *out) {
    if (int rc = test_dev(device_id)) return rc;
    if (int rc = sdp_test_sizes("rqs_inverse", B, 2, T)) return rc;
    std::vector<int> l32;
    if (int rc = glue_test_lens(lens, B, T, l32)) return rc;
    if (!pr || !z || !out || (ch0 != 0 && ch0 != 1) || nb < 1 || nb > 16 || !(sqrt_c > 0.f))
        return fail(nullptr, VITS_E_ARG, "rqs_inverse: null tensor, channel %d, %d bins outside [1, 16] or divisor %g", ch0, nb, (double)sqrt_c);
    const size_t n = (size_t)B * 2 * T;
    DevBufs D;
    const float *dp = D.up(pr, (size_t)B * (3 * nb - 1) * T);
    const int *dlen = D.up(l32.data(), (size_t)B);
    float *dz = up_guarded(D, z, n, (size_t)T);
    TCHECK(D.err);
    launch_rqs_inverse(nullptr, B, T, nb, dp, dz, dlen, ch0, ch0 ^ 1, sqrt_c);
    TCHECK(hipGetLastError());
    TCHECK(hipDeviceSynchronize());
    TCHECK(download(out, dz, n + T));
    return VITS_OK;
}

int vits_test_ea_logw(int device_id, const float *z, int ch, float m0, float logs0, const int64_t *lens, int B, int T, float *out) {
    if (int rc = test_dev(device_id)) return rc;
    if (int rc = sdp_test_sizes("ea_logw", B, 2, T)) return rc;
    std::vector<int> l32;
    if (int rc = glue_test_lens(lens, B, T, l32)) return rc;
    if (!z || !out || (ch != 0 && ch != 1)) return fail(nullptr, VITS_E_ARG, "ea_logw: null tensor or channel %d", ch);
    const size_t n = (size_t)B * T;
    DevBufs D;
    const float *dz = D.up(z, n * 2);
    const int *dlen = D.up(l32.data(), (size_t)B);
    float *dout = D.fill<float>(n + T, 0xff);
    TCHECK(D.err);
    launch_ea_logw(nullptr, B, T, dz, ch, m0, logs0, dlen, dout);
    TCHECK(hipGetLastError());
    TCHECK(hipDeviceSynchronize());
    TCHECK(download(out, dout, n + T));
    return VITS_OK;
}

}  // extern "C"
