/*
 * vitsmi.h — C ABI of libvitsmi.so, the MI355X-native (gfx950) VITS inference engine
 * that replaces the onnxruntime session on phoonnx's hot path.
 *
 * Reference interface replaced (paths relative to the phoonnx checkout):
 *   - session construction      phoonnx/voice.py:167-171  -> vits_open()
 *   - session.get_inputs()      phoonnx/voice.py:347      -> vits_num_inputs()/vits_input_name()
 *   - session.run(None, feed)   phoonnx/voice.py:374-377  -> vits_run()
 * The computation is the graph phoonnx_train/export_onnx.py:250-327 traces from
 * SynthesizerTrn.infer (phoonnx_train/vits/models.py:681-722); weights are read from
 * the same .onnx file onnxruntime would load.
 *
 * Conventions: plain pointers and sizes, no C++ or torch types.  All functions
 * returning int return 0 on success and a negative VITS_E_* code on failure; the
 * message is available from vits_last_error().  A handle owns one HIP stream, the
 * device weight arena and a growable activation workspace; calls on one handle are
 * serialised by an internal mutex, different handles (one per GPU) run concurrently.
 */
#ifndef VITSMI_H
#define VITSMI_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct vits_handle vits_handle;

enum {
    VITS_OK = 0,
    VITS_E_IO = -1,        /* cannot open / read the .onnx file */
    VITS_E_FORMAT = -2,    /* not a VITS graph this engine understands */
    VITS_E_ARG = -3,       /* invalid argument (shape, id out of range, missing sid, ...) */
    VITS_E_DEVICE = -4,    /* HIP error / no gfx950 device */
    VITS_E_NOMEM = -5,
    VITS_E_RANGE = -6      /* f16x3 arithmetic only: an activation left the range of the fp16 operand planes (|x| > 65504,
                              or a non-finite value entered the generator); the engine reports it instead of returning
                              clamped audio.  Reopen with gen_precision "bf16x6" (fp32 range). */
};

/* Stage taps for parity tests ("emb","x","m_p","logs_p","logw","w_ceil","z_p","z"). */
#define VITS_MAX_DIMS 4

/* ---- lifetime ------------------------------------------------------------------- */

/* Parse `onnx_path`, derive the model description, pack the weights into one
 * contiguous device arena on GPU `device_id` (replaces InferenceSession(path, ...),
 * voice.py:167-171). */
int vits_open(const char *onnx_path, int device_id, vits_handle **out);

/* Same, but the packed weight arena is supplied by the caller (already resident on the
 * device, e.g. received by an RCCL broadcast from the rank that read the file, or owned by
 * another handle on the same GPU).  The file is parsed for the model description and the arena
 * LAYOUT only: no weight is packed again.  `arena_dev` must stay valid for the life of the
 * handle.  See vits_arena_* below. */
int vits_open_with_arena(const char *onnx_path, int device_id, void *arena_dev, size_t arena_bytes,
                         vits_handle **out);

/* Host-only open: parses and packs but touches no GPU (device_id ignored).  Only the
 * metadata / arena / hparam calls work on such a handle.  Used by CPU-side tests and
 * by non-root ranks that only need the arena size. */
int vits_open_host(const char *onnx_path, vits_handle **out);

/* Host-only and layout-only: the model description and the arena layout (vits_arena_bytes, vits_hparam,
 * vits_meta) without packing a single weight - exactly what vits_open_with_arena computes before it adopts the
 * caller's device arena.  vits_arena_host() is NULL on such a handle. */
int vits_open_layout(const char *onnx_path, vits_handle **out);

/* Everything above in one call, with the generator's arithmetic chosen explicitly instead of through
 * VITSMI_GEN_PRECISION in the environment. */
typedef struct {
    int device_id;
    const char *gen_precision;  /* NULL / "": environment or default ("f16x3"); "f16x3", "bf16x6", "f16" */
    void *arena_dev;            /* as vits_open_with_arena, or NULL */
    size_t arena_bytes;
    int host_only;              /* as vits_open_host */
    int layout_only;            /* as vits_open_layout (with host_only) */
} vits_open_options;
int vits_open_opts(const char *onnx_path, const vits_open_options *opts, vits_handle **out);

void vits_close(vits_handle *h);

/* Last error message for this handle (or, with h == NULL, of the last failed open on
 * this thread).  Never NULL. */
const char *vits_last_error(vits_handle *h);

/* ---- model description (session.get_inputs(), metadata_props) ---------------------- */

int vits_num_inputs(vits_handle *h);                 /* 3, or 4 with "sid" */
/* "input","input_lengths","scales"[,"sid"]; a third-party graph may also declare "langid" (voice.py:369): it is
 * listed here so that the caller's feed filter (voice.py:373) keeps it, and ignored by the engine (a graph that
 * really consumes a language table is rejected at open). */
const char *vits_input_name(vits_handle *h, int i);

/* metadata_props written by export_onnx.py:335-350 (sample_rate, n_speakers, ...).
 * Returns the value length, or VITS_E_ARG if the key is absent.
 * One key is the loader's own: "vitsmi.name_warnings" - present only when node names and graph structure disagree about
 * which module a Conv belongs to (the names win, the file loads): every such node, one per line. */
int vits_meta(vits_handle *h, const char *key, char *buf, size_t n);

/* Derived hyper-parameters: "hidden","inter","filter","n_heads","n_layers","n_vocab",
 * "n_speakers","gin","use_sdp","hop" (= product of upsample rates),"n_ups","resblock",
 * "gen_sx" (1: the generator runs on the split-operand matrix-core engine, 0: on the f32-MFMA engine),
 * "enc_sx" (1: the text encoder's convs run on the split-operand engine too - f16x3 voices; VITSMI_ENC_ENGINE=f32 keeps
 *   the f32-MFMA engine),
 * "workspace_bytes" (device memory the handle's workspaces hold right now: grows with the largest request, vits_reserve),
 * "gen_rf_frames" (one-sided receptive field of the generator in frames: the context chunked rendering adds),
 * "gen_nprod" (the generator's arithmetic, chosen by VITSMI_GEN_PRECISION in the environment at open time:
 *   2 = "f16x3", the default: fp32 operands as two fp16 planes, three MFMA products per fp32 product, fp32
 *       accumulation; error no larger than the f32-MFMA engine's,
 *   6 = "bf16x6": three bf16 planes, six products, every fp32 product exact to 2^-24,
 *   1 = "f16": BASELINE config 4's reduced-precision vocoder - ONE fp16 plane per operand, one MFMA product per fp32
 *       product, fp32 accumulation, generator activations STORED as fp16 (2 bytes per element instead of 8); everything
 *       in front of z is the default arithmetic.  Range-guarded like f16x3 (VITS_E_RANGE, never clamped audio)). */
int vits_hparam(vits_handle *h, const char *key, int64_t *out);

/* ---- weight arena (multi-GPU: one rank reads + packs, RCCL broadcasts the bytes) ---- */

size_t vits_arena_bytes(vits_handle *h);
/* Host copy of the packed arena (valid until vits_close); NULL for a handle opened with
 * vits_open_with_arena, which never materialises one. */
const void *vits_arena_host(vits_handle *h);
/* Device copy (NULL for a host-only handle). */
void *vits_arena_device(vits_handle *h);

/* ---- the hot call ------------------------------------------------------------------ */

typedef struct {
    /* Optional injected noise for parity with the reference graph's two RandomNormalLike
     * nodes (models.py:111 and :718).  NULL -> generated on the device (Philox) from
     * `seed`.  With scales[2]==0 / scales[0]==0 the respective noise is not used. */
    const float *noise_dp;   /* [B, 2, T] host (vits_run) or device (vits_run_device) */
    const float *noise_z;    /* [B, inter, noise_z_stride] */
    int64_t noise_z_stride;  /* frames per row in noise_z; must be >= max frames */
    uint64_t seed;
} vits_noise;

typedef struct {
    float *data;             /* [B,1,1,S] float32, C-contiguous */
    int64_t dims[4];
    int64_t *y_lengths;      /* [B] frames per utterance (valid samples = y_lengths*hop) */
} vits_output;

/* Host buffers in, host buffers out (what session.run does, voice.py:374).
 *   ids   int64 [B,T]   "input"          (voice.py:350)
 *   lens  int64 [B]     "input_lengths"  (voice.py:351)
 *   scales float32 [3]  [noise_scale, length_scale, noise_w]  (voice.py:364-367)
 *   sid   int64 [B] or NULL              (voice.py:370)
 * `out->data` / `out->y_lengths` are allocated by the library (pinned host memory);
 * release with vits_free_output().  `out` may be NULL: the batch is rendered and kept on the device, to be
 * fetched as 16-bit PCM with vits_last_pcm16() (no fp32 copy to the host at all) together with
 * vits_last_y_lengths(). */
int vits_run(vits_handle *h, const int64_t *ids, const int64_t *lens, int B, int T, const float scales[3],
             const int64_t *sid, const vits_noise *noise, vits_output *out);
void vits_free_output(vits_handle *h, vits_output *out);

/* vits_run without the wait at the end and without an output: host buffers in, the whole path enqueued on the
 * handle's stream.  Returns once the input copies and the one mid-pipeline readback (frame counts:
 * vits_last_y_lengths) are done, i.e. while the generator is still rendering; complete it with vits_fetch_output,
 * vits_last_pcm16 or vits_sync (any of them reports VITS_E_RANGE). */
int vits_run_async(vits_handle *h, const int64_t *ids, const int64_t *lens, int B, int T, const float scales[3],
                   const int64_t *sid, const vits_noise *noise);

/* The last run's waveform -> caller-owned host memory (pageable, or pinned memory from vits_host_alloc for full PCIe
 * rate): row b of the [B, S] result goes to dst + b * row_elems (row_elems >= S; columns [S, row_elems) are zeroed),
 * so that several handles - the sub-batches of one batch, rendered concurrently - can deliver into ONE [B,1,1,S_max]
 * array without a gather on the host.  Typical use: vits_run(..., out = NULL), then vits_last_y_lengths() to size the
 * array, then this.  Waits for the run; VITS_E_RANGE as vits_sync. */
int vits_fetch_output(vits_handle *h, float *dst, size_t row_elems, size_t dst_elems);
/* Pinned (page-locked) host memory for vits_fetch_output / input staging; NULL on failure. */
void *vits_host_alloc(size_t bytes);
void vits_host_free(void *p);

/* Device-resident variant: every pointer (ids, lens, sid, noise arrays) is a device
 * pointer on the handle's GPU; `out->data` and `out->y_lengths` are device pointers into
 * the handle's workspace, valid until the next call on this handle.  Returns after the
 * work has been enqueued on the handle's stream and the one mid-pipeline readback
 * (max frame count) has completed; call vits_sync() before reading `out`. */
int vits_run_device(vits_handle *h, const int64_t *ids, const int64_t *lens, int B, int T,
                    const float scales[3], const int64_t *sid, const vits_noise *noise, vits_output *out);
/* Waits for the handle's stream; VITS_E_RANGE if the run it completes left the fp16 planes' range. */
int vits_sync(vits_handle *h);

/* Chunked (streaming) rendering - SURVEY §8 f1; the reference renders a text sentence by sentence and hands each
 * sentence's audio on as soon as it exists (voice.py:261-269); this does the same INSIDE an utterance batch.
 * Encoder, duration predictor and flow run once; the generator (models.py:348-368) then renders `chunk_frames`
 * frames at a time, each chunk together with vits_hparam "gen_rf_frames" frames of context on either side (the
 * generator's receptive field), of which only the interior is kept: every sample is bit-identical to the one an
 * unchunked vits_run returns.  `fn` is called once per chunk, in order, from the calling thread, while the next chunk
 * renders: samples is host memory [B][n_samples] (row b = utterance b, valid during the call), covering samples
 * [first_sample, first_sample + n_samples) of each row of the [B,1,1,total_samples] output; rows shorter than the
 * longest utterance carry the generator's rendering of their padding, as in vits_run.  A non-zero return stops the
 * run early.  Frame counts: vits_last_y_lengths().  The generator workspace is sized by the chunk, not by the
 * utterance. */
typedef int (*vits_chunk_fn)(void *user, const float *samples, int B, int64_t first_sample, int64_t n_samples,
                             int64_t total_samples);
int vits_run_chunked(vits_handle *h, const int64_t *ids, const int64_t *lens, int B, int T, const float scales[3],
                     const int64_t *sid, const vits_noise *noise, int chunk_frames, vits_chunk_fn fn, void *user);
/* ... and for the vocoder-only entry (z as in vits_run_vocoder). */
int vits_run_vocoder_chunked(vits_handle *h, const float *z, int B, int F, const int64_t *sid, int chunk_frames,
                             vits_chunk_fn fn, void *user);

/* ---- per-utterance synthesis settings ------------------------------------------------
 * Row twins of vits_run_async / vits_run_device / vits_run_chunked: the same arguments, except that
 *   scales  host float32 [B][3]: utterance b's own [noise_scale, length_scale, noise_w]
 *           (models.py:111 noise_w, :702-704 length_scale, :718 noise_scale), also for vits_run_device_rows;
 *   seeds   host uint64 [B], or NULL: utterance b's own 64-bit noise seed.
 * Every value of `scales` must be finite (VITS_E_ARG naming the row, before anything is enqueued); otherwise a row
 * accepts what the [3] vector accepts.  A row equal to the [3] vector with seeds = NULL gives the base function's results
 * bit for bit.  Injected noise (vits_noise.noise_dp / noise_z) takes precedence over the seeds for that tensor.
 *
 * The per-utterance noise stream (seeds != NULL).  Utterance b's noise tensors are those a caller would inject as its
 * row of noise_dp ([2, T], stream 1) and of noise_z ([inter, F], stream 2); element (ch, pos) of tensor `stream` is
 *   (r0, r1, r2, r3) = Philox4x32-10(counter = (pos >> 2, ch, stream, 0), key = (lo32(seeds[b]), hi32(seeds[b])))
 *                      (multipliers 0xD2511F53, 0xCD9E8D57; key increments 0x9E3779B9, 0xBB67AE85; 10 rounds)
 *   u_i = (float)r_i + 0.5f, times 2^-32 (fp32);  u0 and u2 clamped to [1e-12, 1]
 *   v = (sqrt(-2 ln u0) cos(2 pi u1), sqrt(-2 ln u0) sin(2 pi u1), sqrt(-2 ln u2) cos(2 pi u3), sqrt(-2 ln u2) sin(2 pi u3))
 *   noise = v[pos & 3]
 * i.e. a function of (seeds[b], stream, ch, pos) alone: the utterance's place in the batch, the batch's T and F, the
 * handle and the number of calls it has served do not enter.  Its durations and frame count therefore depend on its own
 * inputs only; so do its samples except the last vits_hparam "gen_rf_frames" frames, where the padded batch's generator
 * still sees a longer neighbour's frames (as in vits_run).  Across batch layouts (other B, T) the encoder's sums may
 * differ in their last bits: equal durations, samples within fp32 summation-order distance.  Without seeds, the noise is today's stream: one Philox draw
 * over the whole [B, 2, T] / [B, inter, F] tensor, keyed by vits_noise.seed mixed with a per-handle run counter. */
int vits_run_async_rows(vits_handle *h, const int64_t *ids, const int64_t *lens, int B, int T, const float *scales,
                        const int64_t *sid, const vits_noise *noise, const uint64_t *seeds);
int vits_run_device_rows(vits_handle *h, const int64_t *ids, const int64_t *lens, int B, int T, const float *scales,
                         const int64_t *sid, const vits_noise *noise, const uint64_t *seeds, vits_output *out);
int vits_run_chunked_rows(vits_handle *h, const int64_t *ids, const int64_t *lens, int B, int T, const float *scales,
                          const int64_t *sid, const vits_noise *noise, const uint64_t *seeds, int chunk_frames,
                          vits_chunk_fn fn, void *user);

/* ---- timing control: forced durations and per-token rate ----------------------------------
 * One definition of "duration": durations[b][t] is the integer number of frames token t of utterance b occupies - w_ceil of
 * models.py:702-704 in a free run.  An utterance's frame count is max(1, sum_t durations[b][t]), and sample s belongs to
 * frame s / hop (vits_hparam "hop").
 *
 * vits_controls carries everything a run can be steered with; vits_run_async_ctl / vits_run_chunked_ctl are
 * vits_run_async_rows / vits_run_chunked_rows with the struct in the place of (scales, seeds).  With durations == NULL and
 * token_rate == NULL they compute what those calls compute, bit for bit (they check lens[b] in [0, T] themselves, first).
 *
 * token_rate (host float32 [B][T]): a per-token multiplier on the predicted duration.  Token t < lens[b] of row b gets
 *     w_ceil = ceilf(((expf(logw) * mask) * length_scale) * token_rate[b][t])
 *   in exactly this order of fp32 operations.  So a rate of 1.0 everywhere gives the bits of a run without rates, and with
 *   length_scale == 1.0 a rate r gives the bits the graph gives at length_scale = r.  Rates must be finite and >= 0; rate 0
 *   drops the token (0 frames).  Positions behind lens[b] are ignored.
 * durations (host int64 [B][T]): forced durations.  The duration predictor is NOT launched - neither the stochastic nor the
 *   plain one: none of its convs, spline flows or noise - and one small kernel turns the array into what the free path
 *   leaves behind (w_ceil as float, its inclusive prefix sums, the frame counts).  Everything behind it is the free path
 *   unchanged: the frame-count readback, the expansion of the prior with rows and seeds, flow, generator, ragged tails and
 *   chunking.  A forced run with the durations and seeds of a free run therefore returns that run's frame counts, z_p, z and
 *   waveform bit for bit.  noise_dp, the rows' noise_w and length_scale are accepted and unused; positions behind lens[b]
 *   are ignored (they read 0 afterwards).  After a forced run vits_tap("logw") returns VITS_E_ARG ("not computed in a
 *   forced-duration run"), "w_ceil" gives the forced values, and vits_get_stats reports dp_flops == 0 and the launches
 *   that were made.
 * Validation happens on the host before anything is enqueued or allocated; the error is VITS_E_ARG and names row and
 * token: a negative duration; a duration, or a running row sum, above the frames a forced run admits (below); a non-finite or
 * negative rate;
 * durations together with token_rate (contradictory).  A rejected call leaves the previous run's results readable.
 * Not covered: the device-pointer entries (vits_run_device*), which keep their signatures. */
/* Frames per utterance a forced run admits: min(VITS_MAX_FORCED_FRAMES, INT_MAX / hop).  The first keeps w_ceil exact in
 * fp32 and the frame sums in int; the second keeps the utterance's SAMPLE count (frames * hop) in int as well (at hop 256:
 * 8388607 frames).  A free run is not capped: its length is the model's. */
#define VITS_MAX_FORCED_FRAMES (1 << 24)
typedef struct {
    const float *scales_rows;   /* host [B][3], as vits_run_async_rows; required */
    const uint64_t *seeds;      /* host [B] or NULL */
    const int64_t *durations;   /* host [B][T] or NULL: forced durations */
    const float *token_rate;    /* host [B][T] or NULL: per-token multiplier on the predicted duration */
} vits_controls;
int vits_run_async_ctl(vits_handle *h, const int64_t *ids, const int64_t *lens, int B, int T, const int64_t *sid,
                       const vits_noise *noise, const vits_controls *ctl);
int vits_run_chunked_ctl(vits_handle *h, const int64_t *ids, const int64_t *lens, int B, int T, const int64_t *sid,
                         const vits_noise *noise, const vits_controls *ctl, int chunk_frames, vits_chunk_fn fn, void *user);

/* Frame counts of the last run, from the host copy made by the mid-pipeline readback
 * (no synchronisation).  Writes min(n, B) values, returns B. */
int vits_last_y_lengths(vits_handle *h, int64_t *buf, int n);

/* Durations [B][T] of the last run (free, rate-scaled or forced; the device-pointer runs included), from a host copy made
 * by the same mid-pipeline readback: no synchronisation and no wait, valid as soon as vits_run_async* returns, and the
 * consumer of a chunked run may call it from its callback while later chunks render.  Positions t >= lens[b] read 0;
 * max(1, row sum) is vits_last_y_lengths.  Writes min(n_elems, B * T) values and returns B * T (buf may be NULL to ask for
 * the size); VITS_E_ARG ("no completed run") before the first run, after a vits_reserve or a run that grew the token
 * workspace without completing, and after vits_run_vocoder*, which has no tokens. */
int vits_last_durations(vits_handle *h, int64_t *buf, size_t n_elems);

/* synthesize()'s post-processing on the device, for the LAST run (phoonnx/voice.py:271-282 and AudioChunk,
 * voice.py:88-91): per utterance, over its y_lengths*hop valid samples: peak-normalise (if `normalize`),
 * scale by `volume`, clip, convert to int16 exactly as the NumPy code does.  `out` is host int16 [B, S];
 * samples past an utterance's length are 0. */
int vits_last_pcm16(vits_handle *h, int normalize, float volume, int16_t *out, size_t out_elems);

/* Vocoder only (BASELINE config 2, and teacher-forced parity): z is [B, inter, F] host
 * float32, already masked; output as vits_run. */
int vits_run_vocoder(vits_handle *h, const float *z, int B, int F, const int64_t *sid, vits_output *out);

/* Copy a stage tensor of the LAST run to host: name in {"emb","x","m_p","logs_p","logw",
 * "w_ceil","z_p","z"}; "emb" is emb[ids] * sqrt(hidden) * mask as [B,hidden,T] (models.py:199): the integer
 * gather, bit-exact.  dims receives the shape (rank returned). buf may be NULL to
 * query the shape only. */
int vits_tap(vits_handle *h, const char *name, float *buf, size_t buf_elems, int64_t dims[VITS_MAX_DIMS]);

/* ---- measurement ------------------------------------------------------------------- */

typedef struct {
    double conv_flops;      /* algorithmic FLOPs issued through the conv engine in the last run */
    double conv_bytes;      /* layer-granular bytes (each conv reads input once, writes output once) */
    double dec_flops, dec_bytes;   /* same, HiFi-GAN generator only */
    double flow_flops, enc_flops, dp_flops;
    float conv_ms;          /* HIP-event time of all conv-engine launches (needs timing enabled) */
    float dec_ms, flow_ms, enc_ms, dp_ms, total_ms;
    int conv_launches, total_launches;
    /* the subset of the conv launches that ran on the split-exact bf16 engine (the generator's convs) */
    double sx_flops;
    float sx_ms;
    int sx_launches;
    /* f16x3 range guard (valid after vits_sync / vits_get_stats): every launch that splits fp32 values into fp16
     * operand planes records the largest magnitude it split.  f16_peak_max: the largest over the run (above 65504 =
     * clamped -> f16_saturated = 1 and VITS_E_RANGE); f16_peak_min: the smallest per-launch peak (a whole tensor below
     * ~2^-12 would lose relative precision: planes resolve 2^-36 absolute); f16_tracked: launches recorded. */
    float f16_peak_max, f16_peak_min;
    int f16_tracked, f16_saturated;
    double sx_bytes;        /* layer-granular bytes of the split-engine launches (as conv_bytes) */
} vits_stats;

/* Enable HIP-event timing on the handle's stream: 1 = stage marks plus events around every conv launch (vits_get_stats
 * conv_ms / sx_ms, vits_launch_records; the event records serialise the launches a little), 2 = stage marks only
 * (enc_ms .. total_ms), 0 = off. */
int vits_set_timing(vits_handle *h, int enable);

/* Padded batches (B > 1 with unequal frame counts; the reference itself only ever runs B = 1, voice.py:350-351).  The
 * exported graph does not mask its generator (models.py:348-368, 720): it renders every utterance to the longest one's
 * length, and the samples behind utterance b's end (y_lengths[b] * hop) are the generator's response to zeros.
 *   reference = 0 (default): those samples are NOT rendered.  Every generator launch ends utterance b's tensors
 *       "gen_rf_frames" behind y_lengths[b], so each VALID sample is bit-identical to the padded rendering, and the
 *       output holds 0.0 from y_lengths[b] * hop on.
 *   reference = 1 (or VITSMI_TAILS=reference in the environment at open time): the graph's padded rendering, tails
 *       included - what onnxruntime returns for the same padded feed.
 * Applies to the following runs of this handle (whole and chunked). */
int vits_set_tails(vits_handle *h, int reference);

/* ---- output rate: the waveform delivered at a requested sample rate, resampled on the device -----------------
 * The reference has no counterpart (phoonnx/voice.py writes config.sample_rate into the WAV header and nothing else); like
 * vits_last_pcm16 this is an extension, and the definition below is its specification.
 *
 * The resampled signal.  Rates fi (in) and fo (out), g = gcd(fi, fo), L = fo / g, M = fi / g.  Constants Z = 16,
 * beta = 8.555504641634386, rho = 0.85 (the widely used "kaiser_fast" windowed-sinc parameters).
 *   s = rho * min(1, L / M),  W = Z / s,  K = 2 * ceil(W)
 *   sinc(u) = sin(pi u) / (pi u);  kaiser(u) = I0(beta * sqrt(1 - u^2)) / I0(beta) for |u| < 1, else 0
 *   k(d) = s * sinc(s * d) * kaiser(d / W)                                   (the continuous kernel)
 *   h[p][j] = (float)k(p / L + K / 2 - 1 - j)   for p in [0, L), j in [0, K)  (the table)
 * The table is computed in double on the host and rounded once to fp32; there is no per-phase renormalisation.
 * Row b has n_b valid input samples (y_lengths[b] * hop; F * hop for a vocoder-only run) and N_b = ceil(n_b * L / M) output
 * samples; S_out = max_b N_b.  Output sample n < N_b:
 *   i = floor(n * M / L),  p = (n * M) mod L  (int64 arithmetic),  m0 = i - K / 2 + 1
 *   y[b][n] = sum_{j = 0 .. K-1} h[p][j] * x[b][m0 + j]
 * accumulated in fp32 with fmaf in ascending j, starting from 0.0f, where x[b][m] reads 0 for m < 0 and for m >= n_b -
 * whatever the tails mode left behind n_b - and y[b][n] = 0.0f exactly for n >= N_b.
 * i.e. a row's output depends on its own valid samples alone: neither the batch layout nor vits_set_tails enters, and the
 * whole and the chunked rendering - which share one device function for a sample - agree bit for bit.
 * (In float64 this design passes a tone at 0.3 of the lower rate at amplitude 1 within 1.5e-4 for 22050 -> 8000 / 16000 /
 * 48000 Hz, leaves 2.1 - 2.3e-5 of a tone at 0.6 fo above the output Nyquist, has phase sums within 1.8e-5 of 1 and
 * max_p sum_j |h[p][j]| <= 1.95.)
 * Limits: both rates in [1, 384000]; L * K <= 2^18 table entries (the common targets need at most 16 640; 22050 -> 22051 is
 * refused); N_b must fit in int.  A violation is VITS_E_ARG naming the value, before anything is allocated.
 *
 * vits_set_output_rate: handle state for the following runs, like vits_set_tails.  out_rate == 0 switches resampling off;
 * in_rate <= 0 means the file's "sample_rate" metadata (22050 without it).  out_rate == in_rate is "no resampling": the
 * native path, unchanged.  Host-only and layout-only handles accept it and keep the plan (no table on a device).  With a
 * rate set:
 *   vits_run (out), vits_fetch_output and vits_last_pcm16 deliver the resampled waveform: dims = [B,1,1,S_out], row pitch
 *     rules as before; vits_last_pcm16 takes the peak over the resampled valid samples, then the same fp32 operations;
 *   vits_run_chunked* / vits_run_vocoder_chunked keep the last K input samples of every row on the device between chunks:
 *     after each chunk the callback receives exactly the output samples whose K inputs now all exist, after the last one the
 *     rest (against zeros).  first_sample, n_samples and total_samples (= ceil(F * hop * L / M)) count output-rate samples;
 *     deliveries are contiguous and in order; a chunk that completes no output sample (chunk_frames * hop shorter than the
 *     filter's look-ahead) makes no call.  Concatenated they are the whole run's [B, S_out] bit for bit, for every
 *     chunk_frames >= 1;
 *   vits_last_y_lengths, vits_last_durations and vits_tap are untouched: frames stay frames;
 *   vits_run_device* return VITS_E_ARG ("not covered with an output rate set");
 *   vits_reserve covers the resampled waveform and its 16-bit rendering too.
 * With the rate off, every path executes exactly what it executed before the rate existed. */
int vits_set_output_rate(vits_handle *h, int in_rate, int out_rate);
/* N_b per row of the last run at the CURRENT output rate (y_lengths * hop with the rate off): from host state like
 * vits_last_y_lengths, valid from the same moment.  Writes min(n, B) values, returns B. */
int vits_last_sample_counts(vits_handle *h, int64_t *buf, int n);
/* The plan of a pair of rates - pure host code, no handle, no device: L, M, K (each pointer may be NULL) and, with
 * table != NULL, h as [L][K] floats (table_elems >= L * K).  table == NULL asks for the sizes. */
int vits_resample_plan(int in_rate, int out_rate, int64_t *L, int64_t *M, int64_t *K, float *table, size_t table_elems);

/* ---- output rate per row: each utterance of a batch delivered at its own sample rate ---------------------------
 * A server that batches callers sees telephony at 8 kHz, ASR at 16 kHz and browsers at 48 kHz in one run.  The text below
 * is the specification; it extends the one above and changes nothing of it.
 *
 * The run has B rows, its input rate is fi, row b has its own rate fo_b.
 * Native rows: fo_b == 0 or fo_b == fi.  N_b = n_b and y[b][n] = x[b][n] bit for bit for n < n_b.
 * Resampled rows: every other row, by the definition above unchanged with (L_b, M_b, K_b, h_b) =
 *   vits_resample_plan(fi, fo_b): N_b = ceil(n_b * L_b / M_b); a sample is K_b fmaf in ascending j from 0.0f; the input reads
 *   0 outside [0, n_b).
 * Buffer: S_out = max_b N_b (at least 1); y[b][n] = 0.0f exactly for N_b <= n < S_out.
 * Consequence: row b of a mixed-rate run is row b of the same run under vits_set_output_rate(fi, fo_b), bit for bit - one
 * device function renders a sample, whichever entry launched it; a run whose rows all name one rate is that run; a run whose
 * rows are all native launches nothing and is the native path.
 * Limits: each rate within the limits above; at most VITS_MAX_ROW_RATES distinct resampling rates in a run.  A violation is
 * VITS_E_ARG naming the row and the value, before anything is allocated; a refused call leaves the previous setting in place.
 *
 * vits_set_output_rates: handle state like vits_set_output_rate, which it replaces (and which, called afterwards, replaces
 * it).  in_rate as there.  n_rows == 0 or out_rates == NULL clears the row rates (and nothing else).  Host-only and
 * layout-only handles validate and keep the plans.  A device handle keeps one table per distinct (fi, fo) - taken over
 * from the setting it replaces where the pair is the same, freed otherwise and at close.  With row rates set:
 *   a run of B != n_rows rows is VITS_E_ARG naming both numbers, before anything is staged or enqueued: the previous run
 *     stays readable;
 *   vits_run*, vits_run_async*, vits_run_vocoder, vits_fetch_output, vits_last_pcm16 and every vits_deliver* work as they
 *     stand, on [B][S_out] and the rows' N_b (vits_last_sample_counts);
 *   every chunked entry - vits_run_chunked*, vits_run_vocoder_chunked*, the encoded, shaped and trimmed forms included - and
 *     vits_run_device* return VITS_E_ARG ("not covered with per-row output rates"): the chunk callbacks describe ONE
 *     rectangular timeline (first_sample, n_samples, total_samples for all rows), and rows at different rates do not have one;
 *   every sample-valued field of a delivery is at its row's own rate: leads, trims, fade lengths, envelope points, look-ahead;
 *   a levelled, shaped or limited delivery's sample_rate must equal the rate of the row of every levelled segment
 *     (VITS_E_ARG naming the segment and both rates): deliver once per rate - or per rate and encoding -, naming that
 *     group's rows;
 *   vits_reserve covers the longest row any of the set plans makes.
 * vits_last_sample_counts reports, after a run with row rates, N_b at the rates of THAT run.
 * With no row rates set, every path executes exactly what it executed before they existed. */
#define VITS_MAX_ROW_RATES 8
int vits_set_output_rates(vits_handle *h, int in_rate, const int32_t *out_rates, int n_rows);
/* the rate each row of the last run was delivered at (the voice's own for a native row): host state like
 * vits_last_sample_counts.  Writes min(n, B) values, returns B. */
int vits_last_sample_rates(vits_handle *h, int32_t *buf, int n);

/* ---- intonation: a value in semitones per token, rendered by a time warp on the device -------------------------------
 * VITS has no F0 input.  The engine raises or lowers a token by the classical RESAMPLING shift: token t is rendered longer
 * by r_t = 2^(semitones / 12) (the existing token_rate path) and then played back r_t times faster by a windowed-sinc
 * interpolator of the resampler's design whose speed changes from token to token.  The tempo is what it was, every frequency
 * of the token is multiplied by r_t - the formants move with the fundamental.  Good for a few semitones; it is not PSOLA
 * and preserves no formants.  The reference has no counterpart; the definition below is the specification.  ("pitch" in
 * this code base is a row stride: the control is called semitones, the mechanism the warp.)
 *
 * Constants: Z = 16, beta = 8.555504641634386, rho = 0.85 as the resampler's; R = 512; FB = 16, ONE = 1 << FB.  All
 * position arithmetic is int64: an input position is a Q16 number.
 * Prototype: g(u) = sinc(u) * kaiser(u / Z) for 0 <= u < Z, else 0; the table G[i] = (float)g(i / R), i = 0 .. Z*R + 1,
 *   computed in double and rounded once (G[Z*R] = G[Z*R + 1] = 0).
 * Token t at st = semitones[b][t], finite with |st| <= 12:
 *   r = 2^(st / 12) in double;  step = llrint(r * ONE);  s = rho * min(1, ONE / step) in double;  c = llrint(s * ONE);
 *   Kh = ceil(Z * ONE / c) in integers                    (19 half-taps for st <= 0, 38 at +12)
 * Plan of a row (pure host code; D_t the row's rendered durations in frames, hop): pos = 0 (Q16), n = 0, cum = 0; tokens
 *   behind lens[b] and tokens with D_t == 0 are skipped; for every other token cum += D_t, P = (cum * hop) << FB,
 *   k = ceil((P - pos) / step) (0 if P <= pos), the segment {n0 = n, pos0 = pos, step, c, Kh, k} is recorded, n += k,
 *   pos += k * step.  The overshoot of pos past P is carried into the next token: phase is continuous, nothing is reset.
 *   N_b = n; token t's OUTPUT SPAN is [n0, n0 + k).  A row without a segment has N_b = n_b and is an identity row.
 * Output sample n of a segment: pos = pos0 + (n - n0) * step, i0 = pos >> FB, and for m = i0 - Kh + 1 .. i0 + Kh, ascending:
 *   dq = |(m << FB) - pos|,  v = dq * c,  i = v >> 23,  f = (float)(v & 0x7FFFFF) * 2^-23 (exact),
 *   w = i < Z*R ? fmaf(f, G[i+1] - G[i], G[i]) : 0,  acc = fmaf(w, x[b][m], acc) from 0.0f,
 *   where x[b][m] reads 0 outside [0, n_b);  y[b][n] = (float)(c / 65536.0) * acc.
 *   y[b][n] = 0.0f exactly for n >= N_b; the buffer is [B][S_w], S_w = max(1, max_b N_b).
 * Identity rows: a row whose tokens all have step == ONE is a masked copy - bit for bit its native row, zeros behind n_b.
 * (In float64 with the table's linear interpolation this design passes a tone at 0.15 * min(1, 1/r) cycles per sample at r
 * times its frequency within 1.8e-5 of amplitude 1 for st in {+-1, +-3, +-7, +-12}; the interpolation costs at most
 * 1.6e-6 against the exact kernel; a tone that lands at 0.6 of the output rate leaves 2.2e-5; max s * sum|w| is 1.95,
 * below the 1.98 the tests' tolerance counts with.)
 * Limits: N_b must fit in int; at most T segments per row.  A violation is VITS_E_ARG naming the row and the token; the
 * semitones are checked before anything is enqueued, and a refused call leaves the previous run readable.
 *
 * vits_run_async_warped is vits_run_async_ctl with the intonation on top.
 *   compensate = 1: token t's duration multiplier becomes token_rate[b][t] * (float)r_t (token_rate 1.0f where
 *     ctl->token_rate is NULL) - one fp32 product on the host, then the token_rate path unchanged: the run's durations, frame
 *     counts, z and native waveform are bit for bit those of vits_run_async_ctl with that rate array.  Together with forced
 *     durations it is VITS_E_ARG: forced durations are the rendered ones.
 *   compensate = 0: ctl passes through untouched - the pure warp: a raised token is also shorter.
 *   Not warped: with into == NULL, token_semitones == NULL or every semitone (in front of lens[b]) == 0.0f the call is
 *     vits_run_async_ctl, bit for bit: no warp is planned or launched.
 * The warp runs behind the generator: the plans are built from the host copy of the durations (vits_last_durations'), which
 * exists before the generator is enqueued - no synchronisation is added -, the segment records are uploaded, and one launch
 * writes [B][S_w] into the staging slab, where the resampled waveform of a run with an output rate lives.  Afterwards
 *   vits_last_sample_counts (N_b), vits_fetch_output, vits_last_pcm16 and every vits_deliver* work on the warped buffer as
 *     they stand; vits_last_y_lengths, vits_last_durations and vits_tap stay in frames;
 *   vits_last_token_spans answers k per token.
 * A warped run with an output rate or per-row output rates set is VITS_E_ARG ("not covered with an output rate set") unless
 * vits_set_pitch_at_rate asked for the rate to be folded into step ("pitch at an output rate" below).
 * Out of scope: the device-pointer entries and the vocoder-only chunked ones have no warped
 * form (the chunked entries with tokens: "streamed pitch" below); the speed is constant per token: no glides between tokens here ("pitch contours" below adds them); formants are not preserved;
 * vits_reserve does not count the warped buffer: a warped run grows the staging slab on demand, as any unreserved run does. */
typedef struct {
    int64_t n0;          /* first output sample of the segment */
    int64_t pos0;        /* Q16 input position of that sample */
    int64_t k;           /* output samples: the token's span is [n0, n0 + k) */
    int32_t step;        /* Q16 input samples per output sample */
    int32_t c;           /* Q16 cutoff s */
    int32_t half_taps;   /* Kh */
    int32_t pad_;        /* 0 */
} vits_warp_seg;         /* 40 bytes */
typedef struct {
    const float *token_semitones; /* host [B][T]; positions behind lens[b] ignored */
    int compensate;               /* 1: tempo kept (above); 0: the pure warp */
} vits_intonation;
int vits_run_async_warped(vits_handle *h, const int64_t *ids, const int64_t *lens, int B, int T, const int64_t *sid,
                          const vits_noise *noise, const vits_controls *ctl, const vits_intonation *into);
/* k per token of the last warped run, [B][T] (0 for a dropped token and behind lens[b]): host state, valid as soon as
 * vits_run_async_warped returns.  Writes min(n_elems, B * T) values and returns B * T; VITS_E_ARG after an unwarped run. */
int vits_last_token_spans(vits_handle *h, int64_t *buf, size_t n_elems);
/* The plan - pure host code, no handle, no device.  vits_warp_token: a token's step, cutoff c and half-taps (each pointer may
 * be NULL); VITS_E_ARG for a value that is not finite or outside [-12, 12].  vits_warp_plan: one row of len tokens (semitones
 * NULL: all 0); segs == NULL asks for the counts; spans (nullable) [len] receives k per token; *n_out receives N_b.  Returns
 * the number of segments (<= len), or VITS_E_ARG naming the token. */
int vits_warp_token(float semitones, int64_t *step, int64_t *cutoff, int32_t *half_taps);
int vits_warp_plan(const int64_t *durations, const float *semitones, int len, int hop, vits_warp_seg *segs, int64_t *spans,
                   int64_t *n_out);

/* ---- pitch contours: semitones glide within a token --------------------------------------------------------------------
 * "Intonation" gives a staircase: the speed is constant per token and jumps at every boundary.  Here token t has a START and
 * an END value in semitones and the speed moves linearly from one to the other across the token's output samples - the rise
 * of a question, the fall at a full stop.  Constants, the table G, the sample formula, Q16 positions and int64 arithmetic
 * are those of "intonation", unchanged; this section is the specification of what differs.
 *
 * Token t at st0, st1, each finite with |st| <= 12:  a = llrint(2^(st0 / 12) * ONE), b likewise from st1 (vits_warp_token's
 *   step).
 * Plan of a row: pos, n, cum and the skipping of dropped tokens as in "intonation".  For a kept token P = (cum * hop) << FB;
 *   k = 0 if P <= pos, else L = P - pos and k = ceil(2 L / (a + b)); the record is {n0 = n, pos0 = pos, k, step0 = a,
 *   step1 = b}.  Sample j of the token (0 <= j < k), all integer, floor division of non-negative numerators,
 *   sgn = b >= a ? 1 : -1:
 *     pos_j = pos0 + j * a + sgn * ((|b - a| * j * (j - 1)) / (2 k))
 *     s_j   = a + sgn * ((|b - a| * j) / k)
 *   The next token starts at pos = pos_k (the same formula at j = k), n += k.  The token may end up to 0.75 sample short of P
 *   or under 2 samples past it; that is carried as the overshoot is in "intonation": the next L is measured from where the row
 *   really is, nothing accumulates.  A token with more than 2^23 output samples is VITS_E_ARG (the products stay in int64);
 *   N_b fits in int as before.
 * Cutoff per output sample, from s = s_j in integers:
 *     c = s <= ONE ? 55706 : (17 * 2^32 + 10 s) / (20 s);   Kh = ceil(Z * ONE / c)
 *   For all 98 305 steps in [ONE / 2, 2 ONE] this is the c vits_warp_token derives in double, so a token with a == b has
 *   exactly the step, c, Kh, k and positions of the "intonation" plan.  The sample is that section's formula at pos_j with
 *   c(s_j), Kh(s_j).
 * Properties (asserted by the tests on the engine's records): every increment pos_{j+1} - pos_j and every s_j lies in
 *   [min(a, b), max(a, b)] - positions never decrease and advance by at most two samples per output -; the end of a row is
 *   within 2 samples of cum * hop; with a == b the records reproduce vits_warp_plan's.
 * (In float64 a tone at 0.15 / max(1, r_max) cycles per sample through one long token gliding -12 -> +12, +12 -> -12,
 *   -3 -> +4 or 0 -> +7 comes out as cos(2 pi f0 pos_j / ONE + phase) within 2.1e-5 of amplitude 1; max s * sum|w| over
 *   every step and 128 phases is 1.987, below the 1.99 the tests' tolerance counts with.)
 *
 * vits_run_async_glided is vits_run_async_ctl with the contour on top.
 *   token_semitones NULL: zeros; token_semitones_end NULL: the start values.
 *   If every token in front of lens[b] has st0 == st1 the call IS vits_run_async_warped with those values: the same kernel,
 *     the same launch count, the same bits (all zeros: vits_run_async_ctl).  Otherwise one glide launch takes the place of
 *     the warp launch; everything after it - vits_last_sample_counts, vits_fetch_output, vits_last_pcm16, every
 *     vits_deliver*, vits_last_token_spans - works as after a warped run.
 *   compensate = 1: token t's duration multiplier is token_rate[b][t] * (float)((r0 + r1) * 0.5), r0, r1 the doubles
 *     2^(st / 12): the arithmetic mean, because k = L / mean step.  With equal ends that is (float)r.  The rest of the
 *     compensate contract - the refusal with forced durations, compensate = 0 passing ctl through - is "intonation"'s.
 *   Refusals, all before anything is enqueued, the previous run stays readable: an output rate or per-row rates set ("not
 *     covered with an output rate set"; with vits_set_pitch_at_rate: only a pitched row whose ratio to the native rate lies
 *     outside [1/4, 4], "pitch at an output rate" below); a value that is not finite within [-12, 12], naming token_semitones[b,t] or
 *     token_semitones_end[b,t]; compensate with forced durations; a host-only handle.
 * Chunked runs are "streamed pitch" below, an output rate "pitch at an output rate" below.
 * Out of scope: curves other than linear in the output index; formant preservation; contour positions in time (the Python pitch_contour= places its points by phoneme count); vits_reserve does
 * not count the buffer, as for the warp. */
typedef struct {
    int64_t n0;          /* first output sample of the segment */
    int64_t pos0;        /* Q16 input position of that sample */
    int64_t k;           /* output samples: the token's span is [n0, n0 + k) */
    int32_t step0;       /* a: Q16 input samples per output sample at the token's start */
    int32_t step1;       /* b: ... towards which it moves at the token's end */
    int32_t pad_[2];     /* 0 */
} vits_glide_seg;        /* 40 bytes, as vits_warp_seg */
typedef struct {
    const float *token_semitones;     /* host [B][T] start values; NULL: zeros */
    const float *token_semitones_end; /* host [B][T] end values; NULL: = the start values */
    int compensate;                   /* 1: tempo kept (above); 0: the pure warp */
} vits_contour;
int vits_run_async_glided(vits_handle *h, const int64_t *ids, const int64_t *lens, int B, int T, const int64_t *sid,
                          const vits_noise *noise, const vits_controls *ctl, const vits_contour *contour);
/* The plan - pure host code.  vits_glide_token: a token's two steps and the factor (float)((r0 + r1) / 2) its duration takes
 * under compensate (each pointer may be NULL).  vits_glide_cutoff: c and Kh of a step within [ONE / 2, 2 ONE].
 * vits_glide_plan: vits_warp_plan's sibling (st0 NULL: zeros; st1 NULL: = st0). */
int vits_glide_token(float st0, float st1, int64_t *step0, int64_t *step1, float *rate);
int vits_glide_cutoff(int64_t step, int64_t *c, int32_t *half_taps);
int vits_glide_plan(const int64_t *durations, const float *st0, const float *st1, int len, int hop, vits_glide_seg *segs,
                    int64_t *spans, int64_t *n_out);

/* ---- pitch at an output rate: the rate folded into the warp's step ---------------------------------------------------------
 * vits_set_pitch_at_rate(h, 1) - handle state for the following runs, like vits_set_tails; 0, the default, keeps every pitched
 * entry's refusal "not covered with an output rate set" - makes the pitched entries take an output rate.
 * The warp is a windowed-sinc resampler with a step per token, so a pitched run with an output rate (vits_set_output_rate) or
 * per-row rates (vits_set_output_rates) set renders in ONE filter pass: with the row's plan (L, M) - fo = fi * L / M -
 *   Folded token: step = llrint(2^(st / 12) * (double)M / (double)L * ONE); c and Kh from the step by vits_warp_token's rule.
 *     A gliding token's a and b are the folded steps of st0 and st1; the closed forms and the cutoff rule of "pitch contours"
 *     are used unchanged - the integer rule equals the double rule on all 516 097 steps of [ONE / 8, 8 ONE].
 *   Row plans: those of "intonation" / "pitch contours" given the steps.  P = (cum * hop) << FB stays a NATIVE input position,
 *     the overshoot is carried; n0, k and N_b are then delivered samples: vits_last_token_spans, vits_last_sample_counts, the
 *     fades, per-token volume and alignments work on them as they stand.  compensate is unchanged: the duration multiplier
 *     is r_t without the ratio, because durations are native frames.
 *   Admitted: 1/4 <= M / L <= 4 on every PITCHED row, so steps lie in [ONE / 8, 8 ONE] and Kh <= 151 (c = 6963 at 8 ONE).  A
 *     pitched row at a rate outside that is VITS_E_ARG naming the rates, before anything is enqueued.
 *   A gliding token of a folded plan has at most 2^22 output samples (VITS_E_ARG naming the token): |b - a| < 2^19, so
 *     |b - a| * j * (j - 1) < 2^19 * 2^44 stays inside 64 bits; 2^23 would not.  Plans without a rate keep 2^23.
 *   Identity rows: a row whose tokens all have st == 0 (both ends) is not rendered by the folded plan but by the resampler's
 *     rule, bit for bit the row of a run at that rate without pitch: N_b = ceil(n_b * L / M), token spans the differences of
 *     ceil(cum_t * hop * L / M) clamped to N_b.  An unpitched request does not change because it was batched with a pitched
 *     one.  With L == M everything is "intonation" / "pitch contours".
 * The run makes one launch of the wide kernels (warp_rate_kernel / glide_rate_kernel) from the native waveform into the
 * staging slab in place of the resampler's launch and the warp's; with per-row rates every row is folded by its own (L_b,
 * M_b).  Afterwards everything that works behind a warped run works as it stands, and vits_last_sample_rates answers the
 * output rate(s).
 * (In float64, over 22050 -> 8000 / 11025 / 16000 / 24000 / 44100 / 48000, 16000 -> 8000 / 48000, 24000 -> 8000, 32000 -> 8000
 *   and 8000 -> 32000 at -12, -5, 0, +3 and +12 semitones: max s * sum|w| is 1.947, and a tone at 0.15 * min(1, 1 / step)
 *   cycles per sample lands at step times its frequency within 1.83e-5.)
 * Chunked runs (vits_run_chunked_glided / _enc_glided) with ONE output rate run the warp stage of "streamed pitch" with the folded
 * plan on the native pieces and no resampler stage; total = S_w at the output rate, and pack, shaping, limiter and leading trim
 * work on it unchanged.  The pieces joined are the whole run's [B][S_w], bit for bit.
 * Out of scope: pitch together with a fitted duration; chunked runs with per-row rates ("not covered with an output rate set
 * per row"); the device-pointer entries; ratios outside
 * [1/4, 4]; formant preservation.  vits_reserve does not count the buffer, as for the warp.
 *
 * The plan - pure host code.  vits_warp_token_rate / vits_warp_plan_rate / vits_glide_plan_rate: vits_warp_token /
 * vits_warp_plan / vits_glide_plan with (L, M) folded in (VITS_E_ARG for a ratio outside [1/4, 4]).  vits_glide_cutoff_rate:
 * c and Kh of a step within [ONE / 8, 8 ONE].  vits_glide_pos_rate: pos_j and (step nullable) s_j of one record within the
 * folded limits, 0 <= j <= k.  vits_rate_identity_spans: an identity row's spans [len] (nullable) and N_b from n_in valid
 * input samples. */
int vits_set_pitch_at_rate(vits_handle *h, int on);
int vits_warp_token_rate(float semitones, int64_t L, int64_t M, int64_t *step, int64_t *cutoff, int32_t *half_taps);
int vits_warp_plan_rate(const int64_t *durations, const float *semitones, int len, int hop, int64_t L, int64_t M, vits_warp_seg *segs,
                        int64_t *spans, int64_t *n_out);
int vits_glide_plan_rate(const int64_t *durations, const float *st0, const float *st1, int len, int hop, int64_t L, int64_t M,
                         vits_glide_seg *segs, int64_t *spans, int64_t *n_out);
int vits_glide_cutoff_rate(int64_t step, int64_t *c, int32_t *half_taps);
int vits_glide_pos_rate(const vits_glide_seg *seg, int64_t j, int64_t *pos, int64_t *step);
int vits_rate_identity_spans(const int64_t *durations, int len, int hop, int64_t L, int64_t M, int64_t n_in, int64_t *spans,
                             int64_t *n_out);
/* Streams of a folded plan ("streamed pitch" gives the rules): the emit rule counts with the PLAN's largest Kh - `half`, the
 * largest over every row's records - in place of 38, and n_cap with its least step in place of ONE / 2:
 * n_cap = min(S_w, ceil((piece_samples + half) * ONE / min_step)).  An identity row is the resampler's: ready(X) =
 * min(N_b, ceil((X - K / 2) * L / M)) (0 while X <= K / 2) - every output whose K inputs exist; its step floor(M * ONE / L)
 * joins the least.  A plan without a rate gets exactly the values of vits_warp_emit_end / vits_warp_stream_cap. */
int vits_warp_emit_end_rate(const vits_warp_seg *segs, int n_segs, int64_t n_in, int64_t n_out, int64_t X, int half, int64_t *ready);
int vits_glide_emit_end_rate(const vits_glide_seg *segs, int n_segs, int64_t n_in, int64_t n_out, int64_t X, int half, int64_t *ready);
int vits_identity_emit_end_rate(int64_t L, int64_t M, int64_t K, int64_t n_in, int64_t X, int64_t *ready);
int64_t vits_warp_stream_cap_rate(int64_t piece_samples, int64_t S_w, int64_t min_step, int half);

/* ---- delivery: the last run's audio packed per request on the device - PCM16, G.711, F32, pauses -------------------
 * The reference post-processes and frames every sentence on the host (phoonnx/voice.py:271-282 peak-normalise / volume /
 * clip, :88-91 int16, :307-326 the pause in front of a sentence); this does it for a whole batch in one operation: read the
 * valid samples of the rows of the last run, apply each row's own post-processing, encode, and lay the results out back to
 * back as the byte streams the callers will send.  The definition below is its specification.
 *
 * Input: the last completed run of the handle, through any entry that leaves a whole waveform - vits_run* with or without
 * `out`, vits_run_async*, vits_run_device* after vits_sync, vits_run_vocoder - natively or at an output rate.  Its rows are
 * x[b][0 .. n_b), n_b = what vits_last_sample_counts reports: y_lengths[b] * hop, or the count at the rate the run was
 * resampled to; every row of a vocoder-only run has F * hop samples, or their resampled count.  Whatever lies behind n_b
 * never shows.
 *
 * Plan: G segments, n_streams = J output streams, an encoding (w bytes per element: 2, 1, 1, 4).
 * Layout: stream j holds, for its segments in the order given, lead_samples elements of silence and then n_row elements;
 * N_j = sum (lead + n_row), 0 for a stream without segments.  Streams lie back to back in dst: off_0 = 0,
 * off_{j+1} = off_j + w * N_j, total = off_J.  Silence is the encoding of sample value 0: 00 00 (PCM16), 0xFF (u-law),
 * 0xD5 (A-law), +0.0f (F32).
 * One sample, in fp32, in exactly this order (the operations of vits_last_pcm16):
 *   peak_row = max |x[b][i]| over i < n_b  (0 for n_b = 0)
 *   peak     = peak_row (normalize 1) | max of peak_row over the stream's segments with normalize 2 (normalize 2)
 *   v = x[b][i];  if normalize: v = peak < 1e-8f ? 0.0f : v / peak;  if volume != 1.0f: v = v * volume;  v = min(max(v,-1),1)
 *   F32:   v
 *   PCM16: q = (int16) trunc(min(max(v * 32767.0f, -32767.0f), 32767.0f)), little endian
 *   ULAW:  s = q >> 2 (arithmetic); neg = s < 0; m = (neg ? -s : s) + 33; seg = clamp(floor(log2 m) - 5, 0, 8);
 *          u = seg == 8 ? 0x7F : (seg << 4) | ((m >> (seg + 1)) & 15);  byte = u ^ (neg ? 0x7F : 0xFF)
 *   ALAW:  s = q >> 3; neg = s < 0; m = neg ? -s - 1 : s; seg = clamp(floor(log2 max(m,1)) - 4, 0, 7);
 *          a = (seg << 4) | ((seg < 2 ? m >> 1 : m >> seg) & 15);   byte = a ^ (neg ? 0x55 : 0xD5)
 * (the two G.711 forms equal CPython's audioop.lin2ulaw / lin2alaw, width 2, on all 65 536 int16 values).
 * So: one row per stream, PCM16, is row b of vits_last_pcm16 cut to n_b, bit for bit; a row's bytes depend on that row alone
 * (with normalize 2: on the stream's other rows too); batch layout, tails mode and position in dst do not enter.
 * The device writes only the audio, packed; silence is filled in on the host and never crosses the bus, and the audio
 * arrives with one copy per maximal run of segments without silence between them (no leads: one copy for the batch).
 * Validation happens on the host before anything is enqueued or allocated; VITS_E_ARG, the message naming the segment
 * index and the value: row outside [0, B); a row named twice (naming the second segment); stream outside [0, n_streams);
 * n_streams outside [1, B]; n_segs outside [0, B]; lead_samples outside [0, INT_MAX]; normalize outside 0..2; a non-finite
 * volume; an unknown encoding; dst_bytes < total (the message states the bytes needed); no completed run or a chunked run
 * ("no completed run").  A rejected call leaves the last run deliverable. */
enum { VITS_ENC_PCM16 = 0, VITS_ENC_ULAW = 1, VITS_ENC_ALAW = 2, VITS_ENC_F32 = 3 };   /* w = 2, 1, 1, 4 bytes */
typedef struct {
    int32_t row;           /* source row of the last run; each row in at most one segment */
    int32_t stream;        /* [0, n_streams): a stream is its segments concatenated in the order given */
    int64_t lead_samples;  /* samples of silence in front of this segment, at the delivered rate; [0, INT_MAX] */
    int32_t normalize;     /* 0 none; 1 peak of this row (voice.py:271-277); 2 peak of the stream */
    float   volume;        /* finite */
} vits_segment;
/* pure host code, no handle, no device (like vits_resample_plan): counts [B] -> stream_samples [n_streams], stream_offsets
 * [n_streams + 1] (each nullable), *total_bytes */
int vits_delivery_plan(const int64_t *counts, int B, const vits_segment *segs, int n_segs, int n_streams, int encoding,
                       int64_t *stream_samples, int64_t *stream_offsets, int64_t *total_bytes);
/* the last run, delivered into caller-owned host memory (pageable, or vits_host_alloc); waits for the run; VITS_E_RANGE as
 * vits_last_pcm16; may be called again with another plan or encoding; vits_fetch_output / vits_last_pcm16 / vits_tap still
 * work afterwards.  dst == NULL asks for the layout only (stream_samples, stream_offsets; stream_offsets[n_streams] is the
 * total): the plan is validated against the last run, nothing is enqueued and nothing waited for. */
int vits_deliver(vits_handle *h, const vits_segment *segs, int n_segs, int n_streams, int encoding, void *dst, size_t dst_bytes,
                 int64_t *stream_samples, int64_t *stream_offsets);

/* ---- trimmed delivery: the delivery with the near-silence at either end of a row cut off on the device, and trailing silence ----
 * A VITS voice renders a stretch of near-silence in front of and behind every sentence.  The entries below are vits_deliver
 * with that stretch found by a scan on the device and left out of what is encoded, packed and copied, and with silence
 * behind a segment as well as in front of it.  One vits_trim runs parallel to each vits_segment; the text below is the
 * specification.
 *
 * For a segment on row b with n = n_b valid samples (as in the delivery) and trim t:
 *   peak_all = max |x[b][i]| over i < n, fmaxf semantics; 0 for n = 0
 *   thr      = t.threshold (mode 1) | t.threshold * peak_all, one fp32 product (mode 2)
 *   sample i < n is ACTIVE iff fabsf(x[b][i]) > thr - strictly: a sample equal to the threshold is not active.  Whatever
 *   lies behind n never enters.
 *   mode 0:            a = 0, c = n
 *   no active sample:  a = 0, c = 0
 *   otherwise, f the first and l the last active index:  a = max(0, f - keep_lead), e = min(n, l + 1 + keep_tail),
 *                      c = e - a  (all in int64)
 * The segment contributes lead_samples of silence, the encoded samples x[b][a .. a + c), and tail_samples of silence
 * (silence bytes as in the delivery).  peak_row of the delivery's sample formula is taken over the kept range [a, a + c);
 * normalize 2 takes the max of those kept-range peaks over the stream's normalize-2 segments.  The sample formula and the
 * encoders are unchanged.  N_j = sum (lead + c + tail).
 * So: with trims == NULL, or with every trim at mode 0 and tail_samples 0, the bytes, stream_samples and stream_offsets
 * are vits_deliver's, bit for bit; a row's bytes depend on that row alone (with normalize 2: on the stream's other rows
 * too); tails mode, batch layout and output rate enter only through x and n_b.
 * Device side (csrc/delivery.hip.hpp): delivery_peak_kernel over the untrimmed rows for peak_all (only when a segment uses
 * mode 2), delivery_trim_scan_kernel (min / max of the active indices: order-independent, hence repeatable), one small copy
 * of the bounds to the host, vits_trim_range per segment and the plan there, then the delivery's two kernels over the kept
 * ranges.
 * Validation happens on the host before anything is enqueued or allocated; VITS_E_ARG, the message naming the segment
 * index and the value: mode outside 0..2; a threshold that is not finite or negative; a negative keep_lead or keep_tail;
 * tail_samples outside [0, INT_MAX]; everything vits_deliver refuses.  A rejected call leaves the last run deliverable.
 * Not covered: the encoded stream (its chunks share one first_sample timeline, and a stream cannot know where its audio
 * ends).  Loudness levelling: the next section; fades: the section "shaped delivery" behind it. */
typedef struct {
    int32_t mode;          /* 0 off; 1 absolute: thr = threshold; 2 relative: thr = threshold * peak_all (one fp32 product) */
    float   threshold;     /* finite, >= 0 */
    int32_t keep_lead;     /* samples kept in front of the first active sample, >= 0 */
    int32_t keep_tail;     /* samples kept behind the last active sample, >= 0 */
    int64_t tail_samples;  /* silence behind the segment at the delivered rate, [0, INT_MAX] */
} vits_trim;
/* pure host code: the rule above.  n in [0, INT_MAX]; first_active > last_active means "none active", otherwise
 * 0 <= first_active <= last_active < n. */
int vits_trim_range(int64_t n, int64_t first_active, int64_t last_active, const vits_trim *t, int64_t *a, int64_t *c);
/* pure host code: vits_delivery_plan over kept counts (kept[b]: row b's c), with the tails of trims (nullable) */
int vits_delivery_plan_trimmed(const int64_t *kept, int B, const vits_segment *segs, const vits_trim *trims, int n_segs,
                               int n_streams, int encoding, int64_t *stream_samples, int64_t *stream_offsets, int64_t *total_bytes);
/* vits_deliver with trims [n_segs] (or NULL: none).  Input run, waiting, VITS_E_RANGE and repeatability as vits_deliver.
 * kept_first / kept_count [n_segs] (each nullable) receive every segment's a and c.  The layout depends on the data, so
 * dst == NULL too waits for the run and runs the scan: it reports the layout and the kept ranges, packs nothing and
 * writes to no dst.  dst_bytes < total: VITS_E_ARG, the message states the bytes needed, dst is untouched. */
int vits_deliver_trimmed(vits_handle *h, const vits_segment *segs, const vits_trim *trims, int n_segs, int n_streams, int encoding,
                         void *dst, size_t dst_bytes, int64_t *stream_samples, int64_t *stream_offsets, int64_t *kept_first,
                         int64_t *kept_count);

/* ---- levelled delivery: the trimmed delivery with every segment (or stream) brought to a loudness target on the device ------
 * Peak normalisation makes every sentence equally tall, not equally loud.  The entries below are vits_deliver_trimmed with the
 * integrated loudness of ITU-R BS.1770-4 / EBU R 128 measured on the device over each segment's kept range, turned into ONE gain
 * per segment on the host and applied by the pack launch.  One vits_level runs parallel to each vits_segment; the text below
 * is the specification (tests/loudness_ref.py states it a second time, in float64).
 *
 * For a segment on row b with kept range x[b][a .. a + c) (the trimmed delivery's; a = 0, c = n_b without trims) at the
 * delivered sample rate fs:
 *   K-weighting: two biquads in series, each at rest in front of sample a; coefficients in double on the host, the standard's
 *   analogue prototypes through the bilinear transform (at 48 kHz: the table of BS.1770-4):
 *     shelf      f0 = 1681.974450955533, G = 3.999843853973347 dB, Q = 0.7071752369554196;
 *                K = tan(pi f0 / fs), Vh = 10^(G/20), Vb = Vh^0.4996667741545416, a0 = 1 + K/Q + K^2;
 *                b = [(Vh + Vb K/Q + K^2)/a0, 2 (K^2 - Vh)/a0, (Vh - Vb K/Q + K^2)/a0], a = [1, 2 (K^2 - 1)/a0, (1 - K/Q + K^2)/a0]
 *     high-pass  f0 = 38.13547087602444, Q = 0.5003270373238773; K = tan(pi f0 / fs), a0 = 1 + K/Q + K^2;
 *                b = [1, -2, 1], a = [1, 2 (K^2 - 1)/a0, (1 - K/Q + K^2)/a0]
 *   sub-blocks:  hop = (fs + 5) / 10 samples (integer division); sub-block k is the filtered samples [k hop, (k + 1) hop) of
 *                the kept range, e_k the sum of their squares - an fp32 value from the device; only whole sub-blocks count:
 *                n_sub = c / hop
 *   blocks and gates (host, double): z_j = (e_j + e_{j+1} + e_{j+2} + e_{j+3}) / (4 hop), j = 0 .. n_sub - 4 (400 ms, 75 %
 *                overlap); l_j = -0.691 + 10 log10 z_j; absolute gate l_j > -70; Gamma = -0.691 + 10 log10(mean z over the
 *                absolute-gated blocks) - 10; L = -0.691 + 10 log10(mean z over the blocks with l_j > -70 and l_j > Gamma);
 *                no block, or none that passes: L = -inf
 *   scope:       mode 1 - the segment's own blocks; mode 2 - the blocks of all mode-2 segments of the stream pooled into one
 *                gating computation.  In both the filters restart per row and no block straddles two rows.
 *   gain:        peak = the sample peak of the kept range (mode 2: the max over the stream's mode-2 segments; the quantity
 *                the delivery's normalisation uses - a SAMPLE peak, not a true peak).  L = -inf: g = 1.  Otherwise, in
 *                double: g = 10^((target_lufs - L) / 20); g = min(g, 10^(max_gain_db / 20)); if peak_ceiling > 0 and
 *                peak > 0: g = min(g, peak_ceiling / peak); then rounded once to fp32.
 *   sample:      a levelled segment: v = x[b][i] * g (one fp32 product), then if (volume != 1.0f) v = v * volume, then the
 *                clip; the encoders are unchanged.  Unlevelled segments keep the delivery's formula.
 * So: with levels == NULL, or with every level at mode 0, bytes and layout are vits_deliver_trimmed's, bit for bit.  The
 * layout never depends on the levels.
 * Device side (csrc/loudness.hip.hpp): the kept range is cut into chunks of Lc samples counted from a; every chunk runs the
 * recurrence from rest, the true states are carried through a row's chunks with the 4x4 transition over Lc samples (built in
 * double on the host), every chunk runs again from its true state and sums y^2 per sub-block.  No floating-point atomics, a
 * fixed order of every sum: e_k is bit-identical from call to call and depends on the row's kept samples alone.  Nothing is
 * launched for segments at mode 0.  delivery_peak_kernel supplies the peaks; one small copy brings energies and peaks to the
 * host, which gates, computes the gains and then enqueues the delivery's launches.
 * Validation happens on the host before anything is enqueued or allocated; VITS_E_ARG, the message naming the segment index
 * and the value: mode outside 0..2; a target that is not finite or outside [-70, 0]; max_gain_db not finite or outside
 * [0, 120]; peak_ceiling not finite, negative or above 1 (0: none); a levelled segment whose normalize is not 0; mode-2
 * segments of one stream that disagree in target, max_gain_db or ceiling; with a levelled segment, sample_rate outside
 * [8000, 192000], or differing from the output rate when the handle has one set; everything vits_deliver_trimmed refuses.
 * A rejected call leaves the last run deliverable.
 * Not covered: the encoded stream (it cannot know its integrated loudness in advance; feed a gain in as its volume), true
 * peak, momentary / short-term loudness and loudness range.  Fades: the next section, "shaped delivery". */
typedef struct {
    int32_t mode;          /* 0 off, 1 row, 2 stream */
    float   target_lufs;   /* finite, [-70, 0] */
    float   max_gain_db;   /* finite, [0, 120] */
    float   peak_ceiling;  /* sample-peak ceiling of the levelled segment, (0, 1]; 0: none */
} vits_level;
/* pure host code: the K-weighting of a rate in [8000, 192000] - coef: shelf {b0, b1, b2, a1, a2}, high-pass {b0, b1, b2, a1,
 * a2} - and its hop (each nullable) */
int vits_loudness_filter(int sample_rate, double *coef, int32_t *hop);
/* pure host code: the gates.  e: the sub-block energies of n_rows rows back to back, row r has n_sub[r] >= 0 of them; the
 * rows' blocks are pooled into one gating computation.  L (may be -inf) and the counts of blocks, of blocks that pass the
 * absolute gate, and of blocks that pass both (each nullable). */
int vits_loudness_gate(const float *e, const int32_t *n_sub, int n_rows, int32_t hop, double *L, int32_t *n_blocks, int32_t *n_abs,
                       int32_t *n_rel);
/* pure host code: the gain rule above */
int vits_level_gain(double L, float peak, const vits_level *level, float *gain);
/* pure host code: vits_delivery_plan_trimmed with the levels' validation (levels nullable).  The layout is the trimmed one. */
int vits_delivery_plan_leveled(const int64_t *kept, int B, const vits_segment *segs, const vits_trim *trims, const vits_level *levels,
                               int n_segs, int n_streams, int encoding, int sample_rate, int64_t *stream_samples,
                               int64_t *stream_offsets, int64_t *total_bytes);
/* vits_deliver_trimmed with levels [n_segs] (or NULL: none) at the delivered rate sample_rate.  loudness [n_segs] (nullable)
 * receives every levelled segment's L (mode 2: its stream's; -inf possible), NaN for a segment at mode 0; gain [n_segs]
 * (nullable) every segment's g (mode 0: 1).  dst == NULL measures and reports, packs nothing and writes to no dst. */
int vits_deliver_leveled(vits_handle *h, const vits_segment *segs, const vits_trim *trims, const vits_level *levels, int n_segs,
                         int n_streams, int encoding, int sample_rate, void *dst, size_t dst_bytes, int64_t *stream_samples,
                         int64_t *stream_offsets, int64_t *kept_first, int64_t *kept_count, double *loudness, float *gain);

/* ---- shaped delivery: the levelled delivery with a time-varying volume - fades and per-token gain - applied on the device ------
 * A trimmed segment starts and ends at whatever value the waveform has keep_lead / keep_tail samples away from the threshold
 * crossing: next to the digital silence of a lead, tail or pause that is a step, and through G.711 a click.  And volume can
 * be steered per sentence only (vits_segment.volume), not per word.  Both are one operation, a time-varying `volume`: the
 * entries below are vits_deliver_leveled with a multiplier per sample, computed by the pack launch.  One vits_shape runs
 * parallel to each vits_segment, and all breakpoints of a call live in one array; the text below is the specification
 * (tests/shape_ref.py states it a second time, in NumPy float32), and it is made so that every byte can be checked exactly.
 *
 * vits_env_point.pos is a sample index of the ROW at the delivered rate, counted from the row's start and not from the kept
 * range; it lies in [0, INT_MAX].  vits_env_point.gain is 0, or lies in [2^-20, 64].  fade_in is the number of samples of the
 * kept range that ramp up from 0, fade_out the number that ramp down to 0.
 *
 * For a segment on row b with kept range x[b][a .. a + c) (the trimmed delivery's; a = 0, c = n_b without trims) and points
 * (p_k, g_k), k < m, p strictly ascending:
 *   slopes (host, fp32):  s_k = (g_{k+1} - g_k) / (float)(p_{k+1} - p_k): one fp32 subtraction, one int-to-float conversion,
 *                one correctly rounded fp32 division
 *   envelope at row sample i:  m == 0: e = 1.0f;  i <= p_0: e = g_0;  i >= p_{m-1}: e = g_{m-1};  otherwise, with k the
 *                largest index such that p_k <= i:  e = g_k + s_k * (float)(i - p_k) - the product rounded to fp32, then the
 *                sum rounded to fp32; NOT a fused multiply-add
 *   fades, j = i - a in [0, c):
 *                w_in  = 1.0f if fade_in == 0 or j >= fade_in, else curve((float)j / (float)fade_in)
 *                w_out = 1.0f if fade_out == 0 or c - 1 - j >= fade_out, else curve((float)(c - 1 - j) / (float)fade_out)
 *                curve 0 (linear): curve(t) = t;  curve 1 (smooth): curve(t) = (t * t) * (3.0f - 2.0f * t), each of its four
 *                operations rounded to fp32 separately
 *                So the first and the last kept sample of a faded segment are exactly 0, and fades that overlap
 *                (fade_in + fade_out > c) simply multiply.
 *   multiplier:  mul = (e * w_in) * w_out: two rounded fp32 products
 *   sample:      the existing formula (delivery; levelled delivery) unchanged up to and including
 *                `if (volume != 1.0f) v = v * volume`; then v = v * mul; then the clip and the encoders, unchanged.
 * What the measurements see: the peaks of normalize 1 / 2, the trim scan and the loudness measurement all see the UNSHAPED
 * audio.  A shape is a time-varying volume: like volume, it can drive a sample into the clip.
 * So, because x * 1.0f == x: with shapes == NULL, or with every shape without fades and points, bytes and layout are
 * vits_deliver_leveled's, bit for bit.  The layout never depends on the shapes.
 * Device side (csrc/shape.hip.hpp): delivery_pack_shaped_kernel in the place of delivery_pack_kernel, only when some shape
 * has a fade or a point - every other delivery launches what it launched before.  It reads the envelope as one 16-byte
 * record per interval (position, gain, slope, the next interval's start; slope 0 in front of p_0 and from p_{m-1} on, so
 * that g + s * d is the value above in every case).  Every product, sum, difference and
 * quotient above is one rounded instruction: they are written in functions compiled with floating-point contraction off
 * (csrc/shape.hpp; the same functions run the host rule).  HIP's __fmul_rn / __fadd_rn / __fsub_rn / __fdiv_rn are plain
 * operators to the compiler and do not prevent a contraction to FMA.  The NumPy reference uses plain np.float32 operations.
 * Validation happens on the host before anything is enqueued or allocated; VITS_E_ARG, the message naming the segment index
 * and the value: a negative fade; a curve outside 0..1; a negative n_points; first_point < 0 or first_point + n_points beyond
 * the call's point count; more than 1 << 20 points in a call; a pos outside [0, INT_MAX]; positions of one segment that do
 * not ascend strictly (naming the point); a gain that is not finite, is negative, lies in (0, 2^-20) or is above 64;
 * everything vits_deliver_leveled refuses.  A rejected call leaves the last run deliverable and writes nothing to dst.
 * Not covered: crossfades that overlap two segments (the encoded stream: "shaped streaming" below);
 * PipelinedSession / ShardedSynthesizer on the device path (they take the host fallback, audio_encoding.join_trimmed
 * / join_leveled with shapes=, which gives the same bytes).  A limiter: the next section, "limited delivery". */
typedef struct {
    int32_t pos;           /* row sample index at the delivered rate, [0, INT_MAX] */
    float   gain;          /* 0, or [2^-20, 64] */
} vits_env_point;
typedef struct {
    int32_t fade_in;       /* [0, INT_MAX] */
    int32_t fade_out;      /* [0, INT_MAX] */
    int32_t curve;         /* 0 linear, 1 smooth */
    int32_t n_points;      /* >= 0 */
    int64_t first_point;   /* index of this segment's first point in the call's point array */
} vits_shape;
/* pure host code: the validation above of shapes [n_segs] (nullable: nothing to refuse) over the call's n_points points */
int vits_shape_check(const vits_shape *shapes, int n_segs, const vits_env_point *points, int64_t n_points);
/* pure host code: the multiplier of row sample i of a segment with kept range [a, a + c), a <= i < a + c <= INT_MAX; `points`
 * is the call's array (shape->first_point indexes it) */
int vits_shape_gain(const vits_shape *shape, const vits_env_point *points, int64_t a, int64_t c, int64_t i, float *mul);
/* vits_deliver_leveled with shapes [n_segs] (or NULL: none) over points [n_points].  Input run, waiting, VITS_E_RANGE,
 * dst == NULL and repeatability as vits_deliver_leveled; trims, levels and shapes are each nullable. */
int vits_deliver_shaped(vits_handle *h, const vits_segment *segs, const vits_trim *trims, const vits_level *levels,
                        const vits_shape *shapes, const vits_env_point *points, int64_t n_points, int n_segs, int n_streams,
                        int encoding, int sample_rate, void *dst, size_t dst_bytes, int64_t *stream_samples, int64_t *stream_offsets,
                        int64_t *kept_first, int64_t *kept_count, double *loudness, float *gain);

/* ---- limited delivery: the shaped delivery with a look-ahead peak limiter as the last stage in front of the clip -------------
 * A quiet voice levelled to a loudness target gets a gain that pushes its peaks past full scale, and so does a per-token
 * boost.  vits_level.peak_ceiling answers by capping the gain - the target is then missed -, the clip by flattening the peaks.
 * The entries below are vits_deliver_shaped with a gain per sample that ducks under the peaks instead.  One vits_limit runs
 * parallel to each vits_segment; the text below is the specification (tests/limit_ref.py states it a second time, in NumPy),
 * and it is made so that every byte can be checked exactly whatever parallel algorithm computes it: the gain is integer
 * arithmetic up to one final division - no recursive smoother, no floating-point sum whose order matters.
 *
 * A limited segment (mode 1) has kept range [a, a + c) (the trimmed delivery's) and look-ahead L = lookahead.  u[j], j in
 * [0, c), is the value of the existing sample formula up to and including `v = v * mul`: the levelled gain or the
 * normalisation, the volume, the shape's multiplier - everything in front of the clip.
 *   q[j] (int32): the gain this sample would need on its own, in units of 2^-16.  fabsf(u[j]) <= ceiling: q[j] = 65536.
 *                Otherwise q[j] = (int32) floorf((ceiling / fabsf(u[j])) * 65536.0f): the quotient one correctly rounded fp32
 *                division, its product with 2^16 exact.  (A NaN is not above the ceiling: 65536.)  q[k] = 65536 for every k
 *                outside [0, c): a segment never sees its neighbours, nor the rest of its row.
 *   M[j] = min(q[j], .., q[j + L]), j in [-L, c): the look-ahead.
 *   S[j] = M[j - L] + .. + M[j]: the smoothing, a box of L + 1.  An integer, at most 1025 * 65536: it fits int32.
 *   g[j] = (float) S[j] / (float) ((L + 1) * 65536): one int-to-float conversion (round to nearest even) and one correctly
 *                rounded fp32 division.
 *   sample:      v = u[j] * g[j] (one rounded product), then v = fminf(fmaxf(v, -ceiling), ceiling); then the clip and the
 *                encoders, unchanged.
 * What follows from it:
 *   - every window that enters S[j] contains j, so in exact arithmetic g[j] <= ceiling / |u[j]| and the clamp only absorbs
 *     rounding: no delivered sample of a limited segment exceeds `ceiling` in magnitude;
 *   - where no sample of the segment exceeds the ceiling, S = (L + 1) * 65536 and g = 1.0f: every byte is vits_deliver_shaped's;
 *   - with limits == NULL, or every mode 0, bytes and layout are vits_deliver_shaped's, bit for bit, and exactly the launches
 *     of that entry are made;
 *   - the layout never depends on the limits;
 *   - peaks, the trim scan and the loudness measurement see the UNLIMITED audio, as they see the unshaped one;
 *   - a faded segment still starts and ends at exactly 0;
 *   - the gain begins to fall L samples ahead of a peak and has recovered L samples behind it: the window is symmetric,
 *     2 L + 1 wide.
 * Device side (csrc/limit.hip.hpp): two launches beside the existing ones, only when some segment has mode 1, behind the peak
 * launch.  limit_gain_kernel writes g of every packed element into an fp32 buffer (1.0f in a segment that is not limited): a
 * workgroup stages q of a piece of a segment with a halo of L on either side in LDS - recomputing u of the halo, never
 * reading x outside the kept range -, forms M by doubling minima and S from prefix sums, all int32, then divides.
 * delivery_pack_limited_kernel is the shaped pack's body with the product and the clamp above in front of the clip.  The
 * quotients and products of the rule are the contraction-off functions of csrc/shape.hpp, on the host and on the device.
 * Validation happens on the host before anything is enqueued or allocated; VITS_E_ARG, the message naming the segment index
 * and the value: a mode outside 0..1; reserved != 0; of a limited segment: a ceiling that is not finite, is <= 0 or is > 1, a
 * lookahead outside [1, VITS_LIMIT_MAX_LOOKAHEAD], a |volume| above 1024 (which keeps u finite); everything
 * vits_deliver_shaped refuses.  (An all-zero vits_limit is "off".)  A rejected call leaves the last run deliverable and writes
 * nothing to dst.
 * Not covered (the encoded stream: "shaped streaming" below, with a carry across chunks): a
 * true-peak ceiling (the ceiling holds for the samples, not for the waveform between them); separate attack and release
 * times.  PipelinedSession / ShardedSynthesizer take the host fallback (audio_encoding, limits=: the same bytes). */
#define VITS_LIMIT_MAX_LOOKAHEAD 1024
typedef struct {
    int32_t mode;          /* 0 off, 1 on */
    float   ceiling;       /* (0, 1]: no delivered sample of the segment exceeds it in magnitude */
    int32_t lookahead;     /* L: samples at the delivered rate, [1, VITS_LIMIT_MAX_LOOKAHEAD] */
    int32_t reserved;      /* 0 */
} vits_limit;              /* 16 bytes */
/* pure host code: the validation above of limits [n_segs] (nullable: nothing to refuse) over segs [n_segs] (nullable: the
 * volumes are then not looked at) */
int vits_limit_check(const vits_limit *limits, const vits_segment *segs, int n_segs);
/* pure host code: the rule above for one segment - u [c] the unlimited values of its kept range, g [c] receives the gains;
 * written for clarity, not for speed (c * L steps).  Mode 0: every g is 1. */
int vits_limit_gains(const float *u, int64_t c, const vits_limit *limit, float *g);
/* vits_deliver_shaped with limits [n_segs] (or NULL: none) behind n_points.  Input run, waiting, VITS_E_RANGE, dst == NULL and
 * repeatability as vits_deliver_shaped; trims, levels, shapes and limits are each nullable.  The gain buffer is one float per
 * delivered sample of staging: vits_reserve covers it. */
int vits_deliver_limited(vits_handle *h, const vits_segment *segs, const vits_trim *trims, const vits_level *levels,
                         const vits_shape *shapes, const vits_env_point *points, int64_t n_points, const vits_limit *limits, int n_segs,
                         int n_streams, int encoding, int sample_rate, void *dst, size_t dst_bytes, int64_t *stream_samples,
                         int64_t *stream_offsets, int64_t *kept_first, int64_t *kept_count, double *loudness, float *gain);

/* ---- encoded streaming: a chunked run's chunks post-processed, encoded and masked on the device --------------------------
 * vits_run_chunked* hands every chunk over as fp32 [B][n]; vits_deliver refuses a chunked run.  The two entries below are the
 * chunked runs with the delivery's post-processing and encoders applied per chunk, by one more launch per chunk
 * (csrc/stream_pack.hip.hpp); like the delivery they are an extension, and the text below is their specification.
 *
 * What stays the chunked run's.  Apart from `fmt` and the callback type, vits_run_chunked_enc is vits_run_chunked_ctl and
 * vits_run_vocoder_chunked_enc is vits_run_vocoder_chunked: the same chunks in the same order with the same first_sample /
 * n_samples / total_samples; at an output rate the counts are output-rate samples, through the resampler's carry, and a chunk
 * that completes no output sample makes no call; a non-zero return stops the run; VITS_E_RANGE is reported at the end;
 * vits_last_y_lengths, vits_last_durations and vits_last_sample_counts work as after a chunked run, and vits_deliver still
 * answers "no completed run".
 *
 * Row lengths.  Row b has n_b valid samples - what vits_last_sample_counts reports; F * hop, or its count at the output rate,
 * for every row of a vocoder-only run - and valid[b] = clamp(n_b - first_sample, 0, n_samples).
 * Layout of a chunk.  `bytes` is [B][row_pitch_bytes], row_pitch_bytes = round_up(w * n_samples, 16) (w as in the delivery: 2,
 * 1, 1, 4).  Row b holds valid[b] encoded elements and behind them, up to the pitch, the encoding of sample value 0: 00 00,
 * 0xFF, 0xD5 or +0.0f.  A row that has ended is all silence: what the generator rendered behind a row's end never shows, in
 * either tails mode.  `bytes`, `valid` and `peak` are valid during the call.
 * One sample, in fp32, in exactly this order:
 *   v = x[b][i];  if ref_peak: v = ref_peak[b] < 1e-8f ? 0.0f : v / ref_peak[b] (the correctly rounded division);
 *   if volume[b] != 1.0f: v = v * volume[b];  v = min(max(v, -1), 1);  then the encoders of the delivery section, unchanged
 * i.e. vits_deliver's sample with peak := ref_peak[b] (a stream cannot know its own peak).
 * Running peak.  peak[b] = max |x[b][i]| over the row's valid samples i < first_sample + valid[b], taken before any gain with
 * fmaxf semantics, 0 for an empty row; non-decreasing from chunk to chunk, and after the last chunk the peak vits_deliver's
 * normalize 1 would use.  With fixed seeds, or for a voice calibrated once, a caller feeds a reported peak back as ref_peak:
 * the stream is then the normalised delivery, bit for bit.
 * Validation happens on the host before anything is enqueued or allocated and before the chunked run's own checks; VITS_E_ARG
 * naming the row and the value: fmt == NULL; an unknown encoding; a non-finite volume[b]; a non-finite or negative
 * ref_peak[b].  fn == NULL is allowed, as in vits_run_chunked.  A rejected call makes no callback and leaves the previous
 * run's results readable and deliverable.
 * vits_reserve(B, T, F) covers the device chunk buffer for every chunk_frames <= F. */
typedef struct {
    int32_t encoding;        /* VITS_ENC_* */
    const float *ref_peak;   /* host [B] or NULL: row b is normalised by THIS peak (a stream cannot know its own) */
    const float *volume;     /* host [B] or NULL (= 1.0f) */
} vits_stream_format;
typedef int (*vits_enc_chunk_fn)(void *user, const void *bytes, int B, int64_t row_pitch_bytes, int64_t first_sample,
                                 int64_t n_samples, const int32_t *valid, const float *peak, int64_t total_samples);
int vits_run_chunked_enc(vits_handle *h, const int64_t *ids, const int64_t *lens, int B, int T, const int64_t *sid,
                         const vits_noise *noise, const vits_controls *ctl, const vits_stream_format *fmt,
                         int chunk_frames, vits_enc_chunk_fn fn, void *user);
int vits_run_vocoder_chunked_enc(vits_handle *h, const float *z, int B, int F, const int64_t *sid,
                                 const vits_stream_format *fmt, int chunk_frames, vits_enc_chunk_fn fn, void *user);

/* ---- shaped streaming: the encoded stream with fades, a per-token volume and the look-ahead limiter ------------------------
 * The encoded stream above is what a serving process uses when latency matters, and it lacked what the batch delivery has
 * since "shaped delivery" and "limited delivery": a streamed sentence met the silence of its pause with a step, could not
 * take a per-token volume, and clipped where the delivery ducks.  The two entries below are the two _enc entries with a
 * shaping.  Levelling stays out: a stream cannot know its integrated loudness in advance.  So does a trim against the row's own
 * peak; the leading trim against an absolute threshold, or one relative to ref_peak[b], is "trimmed streaming" below.
 *
 * The rule.  One sample of row b follows the rule of the limited delivery for a segment that keeps the whole row: the kept
 * range is [0, n_b) (a stream does know where it ends: the frame counts are on the host before the first chunk is rendered);
 * peak := ref_peak[b]; there is no level gain.  So fade_out counts back from the row's own end n_b, and the valid elements of
 * a row, joined over the chunks, are the bytes the limited delivery gives for that row - bit for bit, in all four encodings,
 * whatever chunk_frames is.  That equality is the specification; tests/stream_shape_ref.py composes it in NumPy.
 *
 * The shaping.  shapes: one vits_shape per row, or NULL.  points / n_points: the call's breakpoints, row samples at the
 * delivered rate, as in the shaped delivery.  lookahead: one L for the call - 0: no limiter; otherwise within
 * [1, VITS_LIMIT_MAX_LOOKAHEAD].  ceiling: host [B] or NULL - 0: this row is not limited; otherwise within (0, 1].  One L
 * per call keeps a chunk rectangular: a row that is not limited gets g = 1 and the same delay.
 * The plan callback (optional) is called once, on the calling thread, after the durations are on the host and before the
 * first chunk is rendered: durations [B][T] are the frames per token and sample_counts [B] the rows' n_b at the delivered
 * rate (a vocoder run has no tokens: T = 0, durations = NULL).  It may replace shapes, points, n_points and ceiling of
 * `inout` (a copy of the call's shaping; what it points to must live until the run returns) - that is how breakpoints land
 * on the token boundaries of a free-running utterance.  lookahead may not change.  A non-zero return ends the run with
 * VITS_E_ARG.  What it writes is validated like up-front shaping; a refusal there ends the run with VITS_E_ARG and no chunk
 * callback - but the run has begun: the PREVIOUS run's results are then gone, unlike after an up-front refusal.
 *
 * The timeline with lookahead = L > 0.  A rendered piece covers [first, first + n) and delivers
 * [max(first - L, 0), first + n - L); the last piece delivers through total_samples; a piece that completes nothing makes no
 * call (the resampler's rule).  So the first chunk arrives when it arrives today, L samples shorter, and the last one is L
 * samples longer: the latency is L samples of audio, not time.  total_samples does not change.  valid[b] is the clamp of
 * n_b against the delivered range.  peak[b] is the running peak over what has been RENDERED so far: it runs up to L samples
 * ahead of what has been delivered, is still non-decreasing and still final after the last chunk.  With L = 0 the timeline
 * is the encoded stream's.
 *
 * With shaping == NULL, or with no fades, no points, no plan and lookahead == 0, the entries make exactly the launches and
 * bytes of the _enc entries (which forward here with NULL).
 * Device side (csrc/stream_shape.hip.hpp): with L = 0 stream_pack_shaped_kernel, the stream's kernel with the shaped
 * delivery's multiplier in front of the clip; with L > 0 stream_pack_limited_kernel, ONE launch per chunk - a workgroup
 * stages q of a tile of the delivered range with a halo of L on either side, runs the limited delivery's minima and prefix
 * sums in LDS, applies, clamps, encodes and stores whole 16-byte cells - and a small kernel that keeps the last 2 L raw
 * samples of every row for the next chunk (the carry, [B][2 L] floats in two generations).
 * Validation happens on the host before anything is enqueued or allocated; VITS_E_ARG, the message naming the row and the
 * value: everything the shape check refuses (rows in the place of segments); a lookahead outside [0, 1024]; a ceiling that
 * is not finite or lies outside {0} and (0, 1]; a |volume[b]| above 1024 on a limited row; everything the _enc entries
 * refuse.  vits_reserve covers the stream's buffers for L = 1024 and two breakpoints per token.
 * Not covered: trailing trim and loudness in a stream; a look-ahead that differs per row; crossfades between sentences; a
 * true-peak ceiling.  PipelinedSession / ShardedSynthesizer take the host fallback (audio_encoding: the same chunks). */
struct vits_stream_shaping;
typedef int (*vits_stream_plan_fn)(void *user, int B, int T, const int64_t *durations, const int64_t *sample_counts,
                                   struct vits_stream_shaping *inout);
typedef struct vits_stream_shaping {
    const vits_shape *shapes;        /* [B] or NULL; fade_out counts back from the row's own end */
    const vits_env_point *points;    /* the call's breakpoints */
    int64_t n_points;
    const float *ceiling;            /* host [B] or NULL; 0: the row is not limited, else (0, 1] */
    int32_t lookahead;               /* L for the call: 0 no limiter, else [1, VITS_LIMIT_MAX_LOOKAHEAD] */
    int32_t reserved;                /* padding, stated: not read */
    vits_stream_plan_fn plan;        /* or NULL */
    void *plan_user;
} vits_stream_shaping;               /* 56 bytes */
/* pure host code: the validation above of a shaping (nullable: nothing to refuse) over B rows; fmt (nullable) gives the
 * volumes of the limited rows */
int vits_stream_shaping_check(const vits_stream_shaping *shaping, const vits_stream_format *fmt, int B);
/* pure host code: the timeline above - what the rendered piece [first, first + n) of rows of `total` samples delivers */
int vits_stream_emit_range(int64_t first, int64_t n, int is_last, int64_t total, int lookahead, int64_t *e_first, int64_t *e_n);
int vits_run_chunked_enc_shaped(vits_handle *h, const int64_t *ids, const int64_t *lens, int B, int T, const int64_t *sid,
                                const vits_noise *noise, const vits_controls *ctl, const vits_stream_format *fmt,
                                const vits_stream_shaping *shaping, int chunk_frames, vits_enc_chunk_fn fn, void *user);
int vits_run_vocoder_chunked_enc_shaped(vits_handle *h, const float *z, int B, int F, const int64_t *sid,
                                        const vits_stream_format *fmt, const vits_stream_shaping *shaping, int chunk_frames,
                                        vits_enc_chunk_fn fn, void *user);

/* ---- trimmed streaming: the leading silence of a streamed row cut off on the device ----------------------------------------
 * A VITS voice renders near-silence in front of every sentence.  The delivery cuts it off ("trimmed delivery"); a caller of
 * the shaped stream who cuts it off on the host plays a fade-in that started inside what was cut away, and a limiter window
 * that saw it.  The two entries below are the two _shaped entries with one vits_stream_onset per row: the LEADING half of the
 * trim.  The trailing half stays out: a stream learns where its audio ends only at the end, and holding back an unbounded
 * run of quiet samples is a different design - a row keeps everything from its start to n_b.
 *
 * The rule.  onsets: one per row, or NULL - no row is trimmed.  mode 0: the row is not trimmed.  mode 1: thr = threshold.
 * mode 2: thr = threshold * ref_peak[b], one fp32 product - it needs fmt->ref_peak, and is the trimmed delivery's mode 2 with
 * peak_all := ref_peak[b].  (A threshold relative to the row's own peak is what a stream cannot know; these two it can.)
 * A valid sample i < n_b is ACTIVE iff fabsf(x[b][i]) > thr: strict, as in the trimmed delivery, and on the raw sample, before
 * any gain.  f_b is the first active index of the row.  Positions are samples at the delivered rate: the scan sees what the
 * pack stage sees, behind the resampler.
 * Let piece k be the rendered piece in which f_b lies and D_k the first sample that piece delivers - e_first of
 * vits_stream_emit_range for it, whether or not the piece completes anything.  The kept range of row b is [a_b, n_b) with
 *     a_b = max(f_b - keep_lead, D_k)
 * i.e. a stream keeps as much of keep_lead as it has not yet handed over.  f_b >= first_k >= D_k >= 0, so 0 <= a_b <= f_b.
 *   - a_b = max(0, f_b - keep_lead), the delivery's a, whenever f_b lies in the first piece: D_0 = 0.
 *   - the same whenever keep_lead <= lookahead, whatever chunk_frames is: D_k = max(first_k - L, 0) <= max(f_b - L, 0)
 *     <= max(f_b - keep_lead, 0).
 * A trimmed row with no active sample keeps nothing: the delivery's c = 0.
 * One sample of row b follows the limited delivery's rule for a segment with kept range [a_b, n_b): the fades count
 * j = i - a_b against c = n_b - a_b; breakpoints stay row positions; q = 65536 outside the kept range ("a segment never sees
 * ... the rest of its row"); everything in front of a_b is the encoding of 0.
 * What does not change: the timeline, first_sample, n_samples, valid[b], total_samples.  A chunk stays rectangular.
 * The callback gains skip[b]: the number of leading elements of row b in THIS chunk that lie in front of a_b,
 * skip[b] = clamp(a_b - first_sample, 0, valid[b]) - valid[b] while the onset is unknown.  The caller sends
 * row[skip[b] .. valid[b]).  Joined over the chunks those elements are the bytes vits_deliver_limited gives for that row under
 * the trim {mode 1, thr, keep_lead = f_b - a_b, keep_tail >= n_b} - bit for bit, in all four encodings.  That equality is the
 * specification; tests/stream_trim_ref.py composes it in NumPy.  The skips of a row sum to a_b, or to n_b for a row with no
 * onset.
 * peak[b] stays the running peak over ALL valid rendered samples, dropped ones included.  After the last chunk it is still
 * the peak normalize 1 would use over the kept range: every dropped sample is at or below thr, and the kept range holds a
 * sample above it.
 * onsets == NULL or every mode 0: exactly the launches and bytes of the _shaped entries, with skip all 0.  The plan callback
 * of the shaping cannot change onsets.
 * Device side (csrc/stream_trim.hip.hpp): stream_onset_kernel, one launch per rendered piece in front of the pack launch, one
 * workgroup per row - an integer minimum, no atomics, so two runs agree - writes a_b once into start [B] (int32, INT32_MAX:
 * unknown).  The pack kernels read it; a stream with onsets but neither fades, points nor limiter takes the shaped kernel.
 * start travels to the host with the running peaks behind each chunk's bytes, in the same copy; once the host has read that
 * every trimmed row's start is known or the row has ended, the scan is not launched again.
 * Validation on the host before anything is enqueued (the previous run stays readable); VITS_E_ARG naming the row and the
 * value: a mode outside 0..2; a threshold that is not finite or is negative; a negative keep_lead; reserved != 0; mode 2
 * without ref_peak; everything the _shaped entries refuse.  vits_reserve covers the starts and the scan's records.
 * Not covered: the trailing trim and tail_samples; onsets that differ in anything but the three fields; a compacted chunk. */
typedef struct vits_stream_onset {
    int32_t mode;                    /* 0 off, 1 absolute threshold, 2 threshold relative to ref_peak[b] */
    float threshold;
    int32_t keep_lead;               /* samples at the delivered rate kept in front of the onset, where not yet delivered */
    int32_t reserved;                /* must be 0 */
} vits_stream_onset;                 /* 16 bytes */
/* vits_enc_chunk_fn with skip [B] behind valid */
typedef int (*vits_enc_chunk_trim_fn)(void *user, const void *bytes, int B, int64_t row_pitch_bytes, int64_t first_sample,
                                      int64_t n_samples, const int32_t *valid, const int32_t *skip, const float *peak,
                                      int64_t total_samples);
/* pure host code: the validation above of onsets (nullable: nothing to refuse) over B rows; fmt (nullable) says whether
 * there is a ref_peak */
int vits_stream_onset_check(const vits_stream_onset *onsets, const vits_stream_format *fmt, int B);
/* pure host code: the rule above - a = max(f - keep_lead, delivered_before) for an onset at f in a piece that delivers from
 * delivered_before <= f on */
int vits_stream_onset_start(int64_t f, int64_t keep_lead, int64_t delivered_before, int64_t *a);
int vits_run_chunked_enc_trimmed(vits_handle *h, const int64_t *ids, const int64_t *lens, int B, int T, const int64_t *sid,
                                 const vits_noise *noise, const vits_controls *ctl, const vits_stream_format *fmt,
                                 const vits_stream_shaping *shaping, const vits_stream_onset *onsets, int chunk_frames,
                                 vits_enc_chunk_trim_fn fn, void *user);
int vits_run_vocoder_chunked_enc_trimmed(vits_handle *h, const float *z, int B, int F, const int64_t *sid,
                                         const vits_stream_format *fmt, const vits_stream_shaping *shaping,
                                         const vits_stream_onset *onsets, int chunk_frames, vits_enc_chunk_trim_fn fn, void *user);

/* ---- streamed pitch: "intonation" and "pitch contours" in the chunked runs, warped and glided piece by piece -------------------
 * A chunked run renders the native waveform rectangularly: behind a piece, input samples [0, X) of every row exist.  Row b has
 * its plan (vits_warp_seg or vits_glide_seg records, planned as in the two sections above from the durations, which are on the
 * host before the first chunk), n_b valid input samples and N_b output samples; S_w = max(1, max_b N_b).
 *
 * The emit rule (pure host code, int64 as the plans):
 *   ready_b(X) = the number of n < N_b with (pos_n >> FB) + 38 < X, pos_n by the closed form of the row's family.  Positions
 *     never decrease along a row, so it is a prefix count, found by bisection over n.  The bound uses the uniform 38 half-taps
 *     (the most a sample has), not the sample's own Kh: the rule stays monotone for glides, whose Kh changes per sample, and every
 *     float a tile stages exists when the tile runs.  The price is at most 19 samples of latency on audio that is not raised.
 *   A row with X >= n_b is complete: its inputs behind n_b read 0, as in the whole run, and it constrains nothing.
 *   e(X) = min over the rows with X < n_b of ready_b(X); S_w where there is no such row, and on the last piece.
 *   The piece delivers output samples [emitted, e(X)) of ALL rows - one rectangular output timeline, as every chunk callback
 *   describes; rows shorter than the range hold 0.0f behind N_b.  A piece that completes nothing makes no call.
 *   total_samples is S_w.
 * vits_warp_emit_end / vits_glide_emit_end answer the rule for one row: *ready = N_b where X >= n_in, else ready_b(X).  The
 *   records are checked as the test hooks check them; n_out must be the N_b they give (without a record: n_in).
 * Consequence.  At B > 1 the row that needs the most input per output sample - the most raised one - gates the others; when
 *   it ends, one piece may release a long range.  Such a range is handed over in several calls, in order, of at most
 *     n_cap = min(S_w, 2 * (min(chunk_frames, F) * hop + 38))
 *   output samples each (vits_warp_stream_cap): a piece moves every row's bound by chunk_frames * hop inputs, which at the least
 *   step ONE / 2 completes twice as many outputs, and the 38 of the rule may fall on either side.  The ring, the pack scratch and
 *   the limiter carry so stay chunk-sized.  With a look-ahead L a call delivers at most n_cap + L.
 * Device.  The run's native waveform [B][F * hop] is kept in the staging slab (the history: rows at different speeds need
 *   different amounts of past input, without compensate unboundedly much; 25 MB at batch 32 x 768 frames); every piece's interior
 *   is appended by one device-to-device copy, and the window [emitted, e) is rendered by the whole run's kernel launched over
 *   [n_lo, n_hi): the same function renders a sample whichever tile asks for it, so the pieces joined ARE the whole run's
 *   [B][S_w], bit for bit.  Behind it the stages of "encoded / shaped / trimmed streaming" work on the output timeline unchanged:
 *   valid[] and the masks count by N_b, the plan callback receives N_b as sample_counts, vits_stream_emit_range takes S_w.
 *
 * vits_run_chunked_glided is vits_run_chunked_ctl with the contour on top and delivers fp32 pieces;
 * vits_run_chunked_enc_glided is vits_run_chunked_enc_trimmed with it (shaping and onsets nullable: skip is all 0 without onsets).
 *   token_semitones_end == NULL is the warp: one pair of entries covers both sections.  Equal ends launch the warp's kernel,
 *   otherwise the glide's.  All-zero semitones make the call vits_run_chunked_ctl / vits_run_chunked_enc* exactly: the same chunk
 *   ranges, bits and total_launches, no history, no plan.  compensate is "intonation"'s / "pitch contours"'.
 *   Refusals, before anything is enqueued, the previous run stays readable: an output rate or per-row rates set ("not covered
 *   with an output rate set"; with vits_set_pitch_at_rate: per-row rates, "... per row", and one rate whose ratio to the
 *   native rate lies outside [1/4, 4]); a bad value, naming [b,t]; compensate with forced durations; a host-only handle.
 *   vits_last_sample_counts (N_b) and vits_last_token_spans answer from the plan callback on, and after the run.
 * With one output rate set and vits_set_pitch_at_rate on, the plan is the folded one ("pitch at an output rate").
 * Out of scope: pitch with per-row output rates in a chunked run; the vocoder-only chunked entries (no tokens: no warped form);
 * vits_reserve does not count the history; formant preservation. */
int vits_warp_emit_end(const vits_warp_seg *segs, int n_segs, int64_t n_in, int64_t n_out, int64_t X, int64_t *ready);
int vits_glide_emit_end(const vits_glide_seg *segs, int n_segs, int64_t n_in, int64_t n_out, int64_t X, int64_t *ready);
/* n_cap for pieces of piece_samples input samples (chunk_frames * hop) and rows of S_w output samples; VITS_E_ARG below 1 */
int64_t vits_warp_stream_cap(int64_t piece_samples, int64_t S_w);
int vits_run_chunked_glided(vits_handle *h, const int64_t *ids, const int64_t *lens, int B, int T, const int64_t *sid,
                            const vits_noise *noise, const vits_controls *ctl, const vits_contour *contour, int chunk_frames,
                            vits_chunk_fn fn, void *user);
int vits_run_chunked_enc_glided(vits_handle *h, const int64_t *ids, const int64_t *lens, int B, int T, const int64_t *sid,
                                const vits_noise *noise, const vits_controls *ctl, const vits_stream_format *fmt,
                                const vits_stream_shaping *shaping, const vits_stream_onset *onsets, const vits_contour *contour,
                                int chunk_frames, vits_enc_chunk_trim_fn fn, void *user);

/* ---- fitted durations: speech fitted to a requested number of frames --------------------------
 * SSML's <prosody duration>: a line that has to fill, or stay within, a slot.  The model's own rule is
 * d_t = ceil(w_t * length_scale); a fit keeps the rule and looks for THE MULTIPLIER s AT WHICH THE RULE'S OWN FRAME COUNT IS
 * THE TARGET (Adams' apportionment): a fitted run is what the model renders at another length scale, not a proportional
 * rounding with a bias of its own.  Everything behind w is IEEE double and integers, so host, device and a NumPy restatement
 * (tests/fit_ref.py) agree on every bit.
 *
 * Weights.  w_t is the fp32 value the duration kernel hands to ceilf, ((expf(logw) * mask) * length_scale[b]) * token_rate[b][t]
 *   in this order, 0 behind lens[b].  Cleaned: a value that is not finite or not > 0 counts as 0, a value above 2^24 as 2^24.
 * Count.  count_g(s) = sum over the rows b of group g, t < lens[b], of (int64) ceil((double) w_t * s): one double product,
 *   nothing fused into it; the sum is an integer sum, so its order is free.
 * Range.  S = the doubles of [2^-4, 2^4] (positive doubles order like their bit patterns).
 * Groups.  A group is a set of rows of one run that share one s and one target F, the sum of the group's token durations: one
 *   sentence is a group of one row, a text of several sentences rendered as one batch is one group.  Rows of no group
 *   (group[b] = -1) keep what the duration kernel gave them.
 * Mode 1 (exact).  count(2^-4) > F: s* = 2^-4, durations ceil(w s*), VITS_FIT_FLOOR.  Otherwise s* = the largest s of S with
 *   count(s) <= F.  s* = 2^4 and count < F: VITS_FIT_CEIL, nothing more is handed out.  Otherwise R = F - count(s*); the
 *   candidates are the tokens with ceil(w s+) > ceil(w s*), s+ the next double, and the first R of them - ascending row, then
 *   ascending t - take one more frame: VITS_FIT_MET, the group's durations sum to F exactly.  (With w <= 2^24 and s <= 16 one
 *   ulp of s moves a product by less than 2^-25: no token gains two frames between s* and s+, and there are more than R
 *   candidates.)
 * Mode 2 (at most).  count(1.0) <= F: s* = 1.0, durations ceil(w), VITS_FIT_KEPT.  Otherwise mode 1.
 * Per row, as ever: y_len = max(1, row sum), cum the inclusive prefix sums, w_ceil the durations as float.
 * A target equal to the free run's own count reproduces the free run's durations token for token.  A VITS_FIT_FLOOR outcome is
 * not capped (as a free run is not): its rows are as long as ceil(w / 16) makes them.
 *
 * vits_fit: group host int32 [B] in [-1, n_groups), target_frames host int64 [n_groups], mode host int32 [n_groups].  Checked
 * on the host before anything is enqueued or allocated - VITS_E_ARG naming the group or row and the value, the previous run
 * stays readable: 1 <= F <= min(VITS_MAX_FORCED_FRAMES, INT_MAX / hop); mode in {1, 2}; group ids in [-1, n_groups); no group
 * without rows; ctl->durations together with a fit (contradictory); a host-only handle, behind those.
 * vits_run_async_fitted / vits_run_chunked_fitted / vits_run_chunked_enc_fitted are vits_run_async_ctl / vits_run_chunked_ctl /
 * vits_run_chunked_enc_trimmed with a fit: with fit == NULL or every row at -1 each IS that entry - the same bits, the same
 * launches.  A fitted run launches the duration kernel as ever, then one elementwise kernel that writes w and one workgroup
 * per group that overwrites the fitted rows; the per-group results ride in the one mid-run readback, [w_ceil | y_len | fit]:
 * no copy and no synchronisation is added.  vits_tap "w" answers the [B][T] weights after a fitted run ("not computed"
 * after any other).  vits_last_fit: s*, the achieved frames and the status per group of the last run, from host state, valid
 * as soon as the run call returns and from a chunked run's first callback (or its plan callback) on; writes min(n, G) values
 * per array (each may be NULL), returns G; VITS_E_ARG after a run without a fit.
 * vits_fit_plan: the plan without a handle - weights host fp32 [B][T], lens [B] in [0, T]; durations int64 [B][T] (fitted rows
 * only: 0 behind lens[b]; rows of no group are not written), scale / frames / status [n_groups] (each may be NULL).  Targets
 * are bounded by VITS_MAX_FORCED_FRAMES here.
 * Out of scope: a fit together with semitones or contours (no fitted form of the warped and glided entries); tokens exempt
 * from the fit; groups that span runs; the device-pointer entries; the vocoder-only entries. */
enum { VITS_FIT_MET = 0, VITS_FIT_FLOOR = 1, VITS_FIT_CEIL = 2, VITS_FIT_KEPT = 3 };
typedef struct {
    const int32_t *group;           /* host [B]: the row's group, or -1 */
    int n_groups;
    const int64_t *target_frames;   /* host [n_groups] */
    const int32_t *mode;            /* host [n_groups]: 1 exact, 2 at most */
} vits_fit;
int vits_fit_plan(const float *w, const int64_t *lens, int B, int T, const vits_fit *fit, int64_t *durations, double *scale,
                  int64_t *frames, int32_t *status);
int vits_run_async_fitted(vits_handle *h, const int64_t *ids, const int64_t *lens, int B, int T, const int64_t *sid,
                          const vits_noise *noise, const vits_controls *ctl, const vits_fit *fit);
int vits_run_chunked_fitted(vits_handle *h, const int64_t *ids, const int64_t *lens, int B, int T, const int64_t *sid,
                            const vits_noise *noise, const vits_controls *ctl, const vits_fit *fit, int chunk_frames,
                            vits_chunk_fn fn, void *user);
int vits_run_chunked_enc_fitted(vits_handle *h, const int64_t *ids, const int64_t *lens, int B, int T, const int64_t *sid,
                                const vits_noise *noise, const vits_controls *ctl, const vits_stream_format *fmt,
                                const vits_stream_shaping *shaping, const vits_stream_onset *onsets, const vits_fit *fit,
                                int chunk_frames, vits_enc_chunk_trim_fn fn, void *user);
int vits_last_fit(vits_handle *h, double *scale, int64_t *frames, int32_t *status, int n);

/* Size the handle's device workspaces NOW for requests of up to B utterances x T tokens that render up to F frames each
 * (the batch's longest utterance; T = 0 or F = 0 leaves that domain alone).  A run grows a workspace when a request
 * needs more than any before it - hipFree + hipMalloc of tens of GB at batch 32, a device-wide synchronisation that was
 * measured at 0.3 ms to 5 s - so a serving process calls this once at start-up with the largest request it admits (the
 * frame count of a batch depends on the durations the model predicts, i.e. on the noise as well: leave headroom), and no
 * request up to that size allocates device memory afterwards (vits_last_pcm16's int16 staging, vits_deliver's packed
 * buffer and an encoded stream's chunk buffer of such a request included, shaped or not).  onnxruntime has no counterpart (its arena grows the same way, voice.py:167-171 passes default
 * SessionOptions); nothing in the reference needs to call it.
 * INVALIDATES THE LAST RUN'S RESULTS when a workspace actually grows: the device waveform, frame counts and taps of the
 * last run live in those workspaces, so after a growing vits_reserve (or any run that grows one) vits_fetch_output /
 * vits_last_pcm16 / vits_tap return VITS_E_ARG ("no completed run") until the next run, and an out->data / out->y_lengths
 * pointer still held from vits_run_device / vits_run_async must not be read any more.  Fetch first, reserve afterwards. */
int vits_reserve(vits_handle *h, int B, int T, int F);
int vits_get_stats(vits_handle *h, vits_stats *out);

/* One record per conv-engine launch of the last run made with timing enabled, in launch order (call after
 * vits_get_stats, which reads the events): the kernel instantiation as rocprofv3 spells it (without "void vitsmi::"
 * and the argument list), its HIP-event time, algorithmic FLOPs and layer-granular bytes (fp32 input read once +
 * output written once), pipeline stage (0 encoder, 1 duration predictor, 2 flow, 3 generator), shape.  Writes min(n, count)
 * records, returns count. */
typedef struct {
    char kernel[128];
    double flops, bytes;
    float ms;
    int stage;
    int cin, cout, k, dil, t;   /* the conv's shape (a fused pair: its first conv) and input length */
} vits_launch_record;
int vits_launch_records(vits_handle *h, vits_launch_record *buf, int n);

/* The HIP stream the handle launches on (hipStream_t as void*), for callers that want
 * to order their own work or events against it. */
void *vits_stream(vits_handle *h);

/* ---- kernel-level test hooks (used by tests/ to localise parity failures) ------------ */

/* out[B,Cout,T] = conv1d(x[B,Cin,T], w[Cout,Cin,K], bias) through the MFMA conv engine,
 * same padding pad_l/pad_r with pad_l + pad_r == dil*(K-1); flags: bit0 leaky-relu(slope)
 * on the input, bit1 relu on the output.  Host pointers. */
int vits_test_conv1d(int device_id, const float *x, int B, int Cin, int T, const float *w, const float *bias,
                     int Cout, int K, int dil, int pad_l, int flags, float slope, float *out);
/* Kernel tuning: average launch time (ms) of one same-padded conv shape on random data through the
 * engine; ms_out[0] = ms, [1] = tile config used, [2] = channel chunk.  cfg/ck_override < 0 = automatic. */
int vits_bench_conv1d(int device_id, int B, int Cin, int Cout, int T, int K, int dil, int hint, int iters,
                      int cfg_override, int ck_override, float *ms_out);
/* out[B,Cout,T*stride] = conv_transpose1d(x, w[Cin,Cout,K], bias, stride, pad=(K-stride)/2). */
int vits_test_conv_transpose1d(int device_id, const float *x, int B, int Cin, int T, const float *w,
                               const float *bias, int Cout, int K, int stride, float *out);
/* The f32 conv engine (csrc/conv_engine.hip.hpp) with the whole argument set the pipeline's conv() gives it: prologue and
 * epilogue flags, per-utterance bias, residual, old contents of the outputs, row pitches, the second output and the fp16
 * operand planes.  One launch of the engine's own launcher; every pointer is a host pointer.
 *   value = act(conv(pro(x)) + bias + bias_b[b]), then the flag's rule (the EPI_* enum of conv_engine.hip.hpp).
 * Refused with VITS_E_ARG, never launched: what the engine cannot form (see the field comments). */
enum {
    VITS_CONV_PRO_LRELU = 1, VITS_CONV_PRO_MASK = 2, VITS_CONV_EPI_RELU = 4, VITS_CONV_EPI_MASK = 8, VITS_CONV_EPI_RES = 16,
    VITS_CONV_EPI_ACC = 32, VITS_CONV_EPI_DIV = 64, VITS_CONV_EPI_COUPLING = 128, VITS_CONV_EPI_WN = 256,
    VITS_CONV_EPI_WN_FIRST = 512
};
typedef struct {
    int B, Cin, T, Cout;     /* Cout: the module's output channels (a transposed conv: before the pixel shuffle) */
    int K, dil, pad_l;       /* Conv1d: w [Cout][Cin][K]; pad_l + pad_r == dil * (K - 1) */
    int stride;              /* 1 = Conv1d; > 1 = ConvTranspose1d, w [Cin][Cout][K], padding (K - stride) / 2 (dil, pad_l unused) */
    int hint, cfg, ck;       /* tile / chunk: cfg 0..5 and ck > 0 explicitly (refused where the stage does not fit), or
                              * cfg < 0: by the size class `hint` 0..2 as at pack time */
    int flags;               /* VITS_CONV_* */
    float slope, div, oslope, oslope2;  /* PRO_LRELU; EPI_DIV; leaky_relu slope of what out / out2 store (0 or 1 = none) */
    int wn_split;            /* EPI_WN: first skip row; % 32 == 0, <= Cout */
    const float *x;          /* [B][Cin][T] dense; the hook lays it out with x_cstride floats per row, zeros behind T */
    const float *w, *bias;   /* bias [Cout] or NULL */
    const int64_t *lens;     /* [B] in [0, T], or NULL */
    const float *bias_b;     /* [B][bias_b_stride] or NULL; bias_b_stride >= Cout */
    int bias_b_stride;
    const float *res;        /* EPI_RES: [B][Cout][out pitch] (rows as the conv's own, pitch as out) */
    int x_cstride;           /* 0 = T, else >= T */
    int out_cstride;         /* 0 = T * stride; Conv1d: >= T and within the last time tile (the columns behind T are the
                              * launch's to zero); ConvTranspose1d: T * stride only */
    int out_rows, out_row0;  /* out / out2 hold out_rows rows per utterance (0 = Cout), the conv's row 0 is row out_row0:
                              * a window into a wider tensor.  EPI_WN: out_row0 == 0, out_rows >= wn_split and >= Cout - wn_split */
    const float *old_out, *old_out2;  /* previous contents [B][out_rows][T * stride] dense, or NULL: every element, and
                                       * always the pitch columns, start as `sentinel` */
    float sentinel;
    float *out, *out2;       /* [B][out_rows][out pitch] whole, as the launch left them; out2 NULL = no second output
                              * (EPI_WN needs one) */
    int pl_rows;             /* > 0: operand planes of rows [0, pl_rows) of out; % 32 == 0, <= Cout (EPI_WN: <= wn_split),
                              * stride == 1 */
    float *planes_out;       /* [B][pl_rows][T] read back from the two fp16 planes (cells nobody wrote read as 1.0591) */
    char kernel[128];        /* out: the instantiation launched (as in vits_launch_record) */
    int cfg_used, ck_used;   /* out */
} vits_test_conv_epi_args;
int vits_test_conv1d_epi(int device_id, vits_test_conv_epi_args *a);
/* The flow's gate tanh(a[:H]) * sigmoid(a[H:]) on a [B][2H][T] (planar, host): form 0 = wn_gate_kernel, form 1 =
 * wn_gate_blocked_kernel, which reads `a` in the raw cell layout [2H/8][T][8] (H % 8 == 0; the hook lays it out).
 * acts: [B][H][T]. */
int vits_test_wn_gate(int device_id, const float *a, int B, int H, int T, int form, float *acts);
/* Speaker conditioning out[b][r] = bias[r] + W[r][:] . emb_g[clamp(sid[b], 0, n_speakers - 1)][:] (cond_matvec_kernel);
 * emb_g [n_speakers][gin], W [rows][gin], bias [rows] or NULL, out [B][rows]. */
int vits_test_cond_matvec(int device_id, const float *emb_g, int n_speakers, int gin, const int64_t *sid, int B,
                          const float *W, const float *bias, int rows, float *out);
/* The same three hooks through the split-operand engine the generator runs on when all of its channel counts
 * are multiples of 32 (csrc/conv_sx_engine.hip.hpp); needs Cin % 16 == 0 and Cout % 32 == 0.
 * vits_test_conv1d_sx flags: bit0 -> out = leaky_relu(conv, slope) read back from the 16-bit output planes
 * (else the fp32 raw output), bit2 -> residual epilogue with res = x (Cin == Cout), bit3 -> leaky_relu(slope) on the
 * input (raw-input kernels, Cin <= 64; with arithmetic 2: the input plane holds leaky_relu(x) and the residual is
 * recovered from it), bits 4-5 -> arithmetic: 0 bf16x6 (six exact bf16 plane products), 2 f16 (one fp16 plane, one
 * product: the reduced-precision vocoder), 3 f16x3 (two fp16 planes, three products: the generator's default,
 * VITSMI_GEN_PRECISION), bit7 -> the planes are the only output (needs bit0).  vits_test_conv_transpose1d_sx: a negative
 * stride selects f16x3.
 * vits_bench_conv1d_sx dbg bits: 1 no DMA after the first step, 2 no epilogue, 8 residual epilogue, 16 in-kernel
 * cycle breakdown (128-row tiles only), 64 f16 (single plane), 128 f16x3, 256 the v_mfma_f32_32x32x16 main loop even where
 * the 16x16x32 one applies.  ms_out holds 8 floats: [0] ms per launch, [1] tile config, [3..7] with
 * bit 16: s_memtime ticks per pipeline step spent in {LDS wait, DMA wait, barrier, DMA issue, loads + MFMA}. */
int vits_test_conv1d_sx(int device_id, const float *x, int B, int Cin, int T, const float *w, const float *bias,
                        int Cout, int K, int dil, int pad_l, int flags, float slope, float *out);
/* The split-operand engine (csrc/conv_sx_engine.hip.hpp) with the whole argument set the pipeline's conv_sx() gives a
 * generator-form launch: arithmetic, packing options, the run tile, epilogue flags, the residual in each of its three
 * forms, the accumulate operand, per-utterance bias, slopes, per-utterance tensor ends.  One launch of the engine's own
 * launcher; every pointer is a host pointer, tensors are dense [B][C][T] and the hook converts to and from the engine's
 * layouts.
 *   value = conv(leaky_relu(x, islope)) + bias + bias_b[b], + res, + old_out, / div;
 *   out stores leaky_relu(value, oslope), the planes leaky_relu(value, oslope2); utterance b's tensors end at
 *   min(T, (lens[b] + rag_add) * rag_mul) columns (0 for lens[b] == 0): nothing behind is read or written.
 * Both outputs start as `sentinel` (out: as old_out where given), so an element the launch did not write reads back as the
 * sentinel - through the planes: as the value the planes of the sentinel hold.
 * Refused with VITS_E_ARG, never launched: whatever launch_conv_sx() would refuse (see the field comments). */
enum { VITS_SX_EPI_RES = 1, VITS_SX_EPI_ACC = 2, VITS_SX_EPI_DIV = 4, VITS_SX_EPI_NO_RAW_STORE = 8 };
enum { VITS_SX_BF16X6 = 0, VITS_SX_F16X3 = 1, VITS_SX_F16 = 2 };
typedef struct {
    int B, Cin, T, Cout;     /* Cin % 16 == 0, Cout % 32 == 0; Cout: the module's channels (a transposed conv: before the shuffle) */
    int K, dil, pad_l;       /* Conv1d: w [Cout][Cin][K]; pad_l + pad_r == dil * (K - 1) */
    int stride;              /* 1 = Conv1d; > 1 = ConvTranspose1d, w [Cin][Cout][K], padding (K - stride) / 2 */
    int precision;           /* VITS_SX_BF16X6 / F16X3 / F16 (one fp16 plane; Cin % 32 == 0) */
    int force16, no_s16, min_cfg;  /* SxPack: the 16x16x32 packing also for <= 64 input channels; never that packing;
                                    * smallest tile index */
    int run_cfg;             /* -1: the packed tile; else the tile the launch runs on (the packed one is passed as pack_cfg):
                              * no taller than the packed one, 3 only on the 16x16x32 loop, raw input only on its own */
    int flags;               /* VITS_SX_EPI_*; NO_RAW_STORE: out is only the accumulate operand */
    const float *x;          /* [B][Cin][T] */
    const float *w, *bias;   /* bias [Cout] or NULL */
    const float *res;        /* EPI_RES: [B][Cout][T * stride] fp32, or (res_planes) uploaded as the operand planes of
                              * leaky_relu(res, res_slope) and un-activated on the way in (fp16 arithmetics, plane input; the
                              * single-plane arithmetic has no other form) */
    int res_is_x;            /* EPI_RES instead: the residual is the raw input's own device tensor (raw-input convs, Cin == Cout) */
    int res_planes;
    float res_slope;
    const float *old_out;    /* [B][Cout][T * stride] previous contents of out (the EPI_ACC operand), or NULL */
    const float *bias_b;     /* [B][bias_b_stride] or NULL; bias_b_stride >= Cout */
    int bias_b_stride;
    float div, oslope, oslope2, islope;  /* EPI_DIV; slopes of what out / the planes store and of the raw-input prologue
                                          * (0 or 1 = none; islope on raw-input convs only) */
    const int64_t *lens;     /* [B] in [0, T], or NULL: every utterance spans T */
    int rag_add, rag_mul;    /* SxRagged::add / mul; rag_mul >= 1 */
    float sentinel;
    float *out;              /* [B][Cout][T * stride] as the launch left it, or NULL = no raw tensor */
    float *planes_out;       /* [B][Cout][T * stride] read back from the output planes, or NULL = no plane output */
    float *res_seen;         /* nullable, res_planes: leaky_relu(res, res_slope) as the residual planes hold it */
    char kernel[128];        /* out: the instantiation launched (as in vits_launch_record) */
    int pack_cfg, run_cfg_used, rawin, s16, ck;  /* out: what pack_conv_sx chose, the tile launched */
    float peak;              /* out, fp16 arithmetics: the largest of the launch's 64 range-guard slots (SxArgs::peak) */
} vits_test_conv_sx_epi_args;
int vits_test_conv1d_sx_epi(int device_id, vits_test_conv_sx_epi_args *a);
/* The planar epilogue of the split-operand engine (f16x3 arithmetic, 16x16x32 loop; "same" padding), as the flow's
 * res_skip / pre / post convs and the text encoder's convs use it: o = old + act(conv(x) + bias) * mask, rows
 * [0, row_split) into a first planar tensor, the rest into a second.  flags: 1 ReLU, 2 mask (t < lens[b]), 4 residual
 * (old [B][row_split][T] is added to the first tensor's rows), 8 accumulate (old [B][Cout][T] = the outputs' previous
 * contents), 16 coupling update o = (old - value * mask) * mask (with 8), 32 the second tensor's rows are stored, not
 * accumulated (with 8), 64 the operand planes are those of the second tensor's rows.  out: [B][Cout][T]; planes_out
 * (nullable): [B][pl_rows][T] as read back from the fp16 operand planes the epilogue wrote. */
int vits_test_conv1d_sx_planar(int device_id, const float *x, int B, int Cin, int T, const float *w, const float *bias,
                               int Cout, int K, int dil, int flags, const int64_t *lens, const float *old, int row_split,
                               int pl_rows, float *out, float *planes_out);
/* A/B hook: largest conv launch (workgroups of csrc/conv_sx_small.hip.hpp's kernel) that takes the short-launch kernel;
 * 0 = never (process-wide; default 1536 or VITSMI_SX_SMALL_MAX).  Returns the previous value. */
long long vits_test_set_sx_small_max(long long wgs);
/* The WN in-layer conv with the gate epilogue (tanh(a + g_a) * sigmoid(b + g_b)): w / bias in the packed row order (32 tanh
 * rows, their 32 sigmoid partners, ...), bias_b [B][Cout] in the module's order; flags bit 0: the short-launch kernel, bit 1:
 * the result through the fp16 operand planes.  out: [B][Cout / 2][T]. */
int vits_test_conv1d_sx_gate(int device_id, const float *x, int B, int Cin, int T, const float *w, const float *bias,
                             const float *bias_b, int Cout, int K, int dil, int flags, float *out);
int vits_test_conv_transpose1d_sx(int device_id, const float *x, int B, int Cin, int T, const float *w,
                                  const float *bias, int Cout, int K, int stride, float *out);
int vits_bench_conv1d_sx(int device_id, int B, int Cin, int Cout, int T, int K, int dil, int dbg, int iters,
                         float *ms_out);
/* Two dependent convs of a ResBlock in one fused launch on a raw-format stage (csrc/conv_sx_pair.hip.hpp), C in {32, 64},
 * f16x3 arithmetic, c1 = Conv1d(C, C, K, dilation dil1), c2 = Conv1d(C, C, K, dilation dil2), both "same"-padded:
 *   (chain & 1) == 0 (ResBlock1 step):   out = c2(leaky_relu(c1(leaky_relu(x, slope)), slope)) + x
 *   (chain & 1) != 0 (two ResBlock2 steps): x1 = c1(leaky_relu(x, slope)) + x ; out = c2(leaky_relu(x1, slope)) + x1
 * chain bits 1-2 choose the kernel: 0 conv_sx_pair_kernel, 1 conv_sx_pair16_kernel in f16x3, 2 the same in the single-plane
 * arithmetic; bit 3 (pair16 only): out is read back from the output planes, leaky_relu(result, slope).  The pair16 forms are
 * vits_test_conv_pair16_epi's launch with `raw` or `planes`, no lens, buffers that start as zeros.
 * ms_out (nullable): average launch time over 10 launches. */
int vits_test_conv_pair_sx(int device_id, const float *x, int B, int C, int T, const float *w1, const float *b1,
                           const float *w2, const float *b2, int K, int dil1, int dil2, int chain, float slope, float *out,
                           float *ms_out);
/* conv_sx_pair_kernel with the whole argument set the generator's conv_sx_pair() gives it: one launch of the kernel's own
 * launcher, its arguments filled by the function the generator fills them with.  Every pointer is a host pointer, tensors are
 * dense [B][C][T]; convs, `chain` (0 / 1) and `slope` as vits_test_conv_pair_sx.  Utterance b's tensors end at end_b = lens[b]
 * columns (T without lens): x and c1's result are zero at columns >= end_b, and those columns of out are not written.
 *   value = (the step's result) [+ out_init (ACC)] [/ div (DIV; only with ACC)]
 * out starts as out_init, else as zeros.  Refused with VITS_E_ARG, never launched: what sx_pair_supported() refuses, ACC
 * without out_init, lens outside [0, T]; what launch_conv_sx_pair() itself refuses comes back as VITS_E_DEVICE. */
enum { VITS_PAIR_EPI_ACC = 1, VITS_PAIR_EPI_DIV = 2 };
typedef struct {
    int B, C, T, K, dil1, dil2, chain;
    int flags;               /* VITS_PAIR_EPI_* */
    float slope, div;
    const float *x;          /* [B][C][T] */
    const float *w1, *b1, *w2, *b2;  /* w [C][C][K]; b [C] or NULL */
    const int64_t *lens;     /* [B] in [0, T], or NULL: every utterance spans T */
    const float *out_init;   /* [B][C][T] previous contents of the raw tensor (the ACC operand), or NULL */
    float *out;              /* [B][C][T] the raw tensor as the launch left it */
    char kernel[128];        /* out: the instantiation launched (as in vits_launch_record) */
    int BNo;                 /* out: kept columns per tile */
} vits_test_conv_pair_sx_epi_args;
int vits_test_conv_pair_sx_epi(int device_id, vits_test_conv_pair_sx_epi_args *a);
/* The identity the fused low-plane form rests on, evaluated on the host (_Float16 / fmaf; no device): with v = x clamped to
 * +-65504 and h0 = f16(v), old = f16((v - h0) * 2048) and fused = f16(fmaf(h0, -2048, v * 2048)) as fp16 bits.
 * _sweep: the same over the fp32 bit patterns first, first + 1, .. (count of them; wraps at 2^32): returns the number that
 * differ (NaN against NaN counts as equal), the first one in *first_bad (nullable). */
int vits_test_split_identity(const float *x, int64_t n, uint16_t *h1_old, uint16_t *h1_fused);
int64_t vits_test_split_identity_sweep(uint32_t first, uint64_t count, uint32_t *first_bad);
/* The activation -> operand-plane helpers of csrc/sx_split.hip.hpp on n host values (n even; pair i = values 2 i, 2 i + 1):
 * a = leaky_relu(x, slope) as the fused ResBlock-step kernel computes it, clamped to +-65504, split into h0 = f16(a) and
 * h1 = f16((a - h0) * 2048).  form 0: the engine-wide split; form 1: the one conv_sx_pair_kernel uses.  h0, h1 [n]: the planes'
 * fp16 bits; pk [n / 2]: the range guard's magnitude of each pair, max(|a|, |b|) before the clamp; rec [n]: h0 with the
 * leaky-ReLU undone (v < 0 ? v * (1 / slope) : v). */
int vits_test_split_forms(int device_id, const float *x, int n, float slope, int form, uint16_t *h0, uint16_t *h1, float *pk,
                          float *rec);
/* The fused ResBlock step (csrc/conv_sx_pair16.hip.hpp, conv_sx_pair16_kernel) with the whole argument set the generator's
 * conv_sx_pair16() gives it: one launch of the kernel's own launcher, its arguments filled by the function the generator
 * fills them with.  Every pointer is a host pointer, tensors are dense [B][C][T]; c1 = Conv1d(C, C, K, dilation dil1),
 * c2 = Conv1d(C, C, K, dilation dil2), both "same"-padded; utterance b's tensors end at end_b = min(T, (lens[b] + rag_add) *
 * rag_mul) columns (0 for lens[b] == 0; T without lens):
 *   x is zero at columns >= end_b, whatever the planes hold there
 *   c1 = conv(leaky_relu(x, slope), w1) + b1;  chain == 0: mid = c1, res = x;  chain != 0: mid = c1 + x, res = mid
 *   mid is zero at columns >= end_b;  value = conv(leaky_relu(mid, slope), w2) + b2 + res, + old_out (ACC), / div (DIV)
 *   RAW: out stores value;  PLANES: the planes store leaky_relu(value, slope);  columns >= end_b are not written.
 * The input is uploaded as the operand planes of leaky_relu(x, slope); where x_tail is given, its values (activated the same
 * way) replace x at columns >= end_b.  out starts as old_out, else as `sentinel`; the planes start as the sentinel's split;
 * both carry a guard band of sentinel cells behind the last utterance.
 * Refused with VITS_E_ARG, never launched: what sx_pair16_plan() refuses, ACC without old_out, lens outside [0, T]; what
 * launch_conv_sx_pair16() itself refuses (DIV without ACC, ..) comes back as VITS_E_DEVICE. */
enum { VITS_P16_EPI_ACC = 1, VITS_P16_EPI_DIV = 2, VITS_P16_EPI_RAW = 4, VITS_P16_EPI_PLANES = 8 };
typedef struct {
    int B, C, T, K, dil1, dil2, chain;
    int precision;           /* VITS_SX_F16X3 or VITS_SX_F16 */
    int flags;               /* VITS_P16_EPI_* */
    float slope, div, sentinel;
    const float *x;          /* [B][C][T] */
    const float *w1, *b1, *w2, *b2;  /* w [C][C][K]; b [C] or NULL */
    const float *old_out;    /* [B][C][T] previous contents of the raw tensor (the ACC operand), or NULL */
    const float *x_tail;     /* [B][C][T] or NULL: what the input planes hold at columns >= end_b instead of x */
    const int64_t *lens;     /* [B] in [0, T], or NULL: every utterance spans T */
    int rag_add, rag_mul;    /* SxRagged::add / mul; rag_mul >= 1 */
    float *out;              /* [B][C][T] the raw tensor as the launch left it (nullable) */
    float *planes_out;       /* [B][C][T] read back from the output planes (nullable) */
    float *x_seen;           /* [B][C][T] nullable: x as the kernel recovers it from the input planes (leaky_relu undone) */
    float *ms_out;           /* nullable: average launch time over 10 more launches */
    char kernel[128];        /* out: the instantiation launched (as in vits_launch_record) */
    int BN, BNo, ovl;        /* out: tile columns, kept columns per tile, whether Y overlays the x tile */
    float peak;              /* out: the largest of the launch's 64 range-guard slots (SxPair16Args::peak) */
    int guard_ok;            /* out: the guard bands behind both outputs, and the planes' unused third, kept their bits */
} vits_test_conv_pair16_epi_args;
int vits_test_conv_pair16_epi(int device_id, vits_test_conv_pair16_epi_args *a);
/* Relative-position multi-head self-attention core (attentions.py:225-272): q,k,v
 * [B,C,T] host, emb_rel_k/v [2w+1, dk], lens int64[B]; out [B,C,T]. */
int vits_test_attention(int device_id, const float *qkv, int B, int C, int T, int n_heads, const float *rel_k,
                        const float *rel_v, int window, const int64_t *lens, float *out);
/* ... the f16x3 16x16x32 kernel (kernel = 1; head width 32 / 64 / 96) or the fp32-MFMA one (kernel = 0): out_planes (may be
 * NULL) receives the output's fp16 operand planes [B][3][C/8][T][8]; reps > 0 times reps launches into ms_out[0] (ms each). */
int vits_test_attention16(int device_id, const float *qkv, int B, int C, int T, int n_heads, const float *rel_k,
                          const float *rel_v, int window, const int64_t *lens, float *out, uint16_t *out_planes, int kernel,
                          int reps, float *ms_out);
/* ... either kernel in the form and the instantiation the caller names.  VITS_E_ARG for a (head width, ns, qt, kh) that has no
 * compiled instantiation, for a head wider than 128 channels and for a window above 4: nothing falls back to a neighbour. */
typedef struct {
    int kernel;              /* 16: attention16 (head width 32 / 64 / 96); 32: the fp32-MFMA kernel (head width <= 128) */
    const float *qkv;        /* [B][3 C][T] host; may be NULL for kernel 16 when qkv_planes is given */
    const uint16_t *qkv_planes; /* kernel 16 only, nullable: [B][3][3 C / 8][T][8] operand planes used as they are (otherwise
                              * qkv is split on the device, as the q|k|v conv's epilogue does) */
    int B, C, T, n_heads, window;
    const float *rel_k, *rel_v;  /* [2 window + 1][C / n_heads] */
    const int64_t *lens;     /* [B] >= 0; a length above T counts as T */
    int want_out;            /* the launch writes the fp32 output (kernel 32 always does: 0 is refused there) */
    int want_planes;         /* the launch writes the output's operand planes and the range-guard peak (C % 8 == 0; kernel 32:
                              * head width % 8 == 0) */
    int ns, qt;              /* kernel 16: LDS stages / query tiles per wave; 0 = the launcher's own choice */
    int kh;                  /* kernel 32: key halves (1 / 2); 0 = the launcher's own choice */
    float *out;              /* [B][C][T], nullable: the device buffer as the launch left it; it starts as 0xff bytes */
    uint16_t *out_planes;    /* [B][3][C / 8][T][8], nullable: likewise (the third slot is never written) */
    float peak;              /* out: the largest of the launch's 64 range-guard slots, cleared in front of the launch */
    char kernel_name[128];   /* out: the instantiation launched (as in vits_launch_record) */
} vits_test_attention_form_args;
int vits_test_attention_form(int device_id, vits_test_attention_form_args *a);

/* The resampler by value: x [B][S] host, lens [B] the rows' valid samples (what lies behind must not show), y [B][S_out]
 * with S_out >= max_b ceil(lens[b] * L / M); every column of y is written. */
int vits_test_resample(int device_id, const float *x, const int64_t *lens, int B, int S, int in_rate, int out_rate, float *y,
                       int64_t S_out);
/* ... the same input through the chunked entry, piece_samples input samples at a time (S_out >= ceil(S * L / M)).  Returns
 * the number of deliveries; ranges (nullable, max_ranges pairs) receives each one's (first_sample, n_samples). */
int vits_test_resample_pieces(int device_id, const float *x, const int64_t *lens, int B, int S, int in_rate, int out_rate,
                              int piece_samples, float *y, int64_t S_out, int64_t *ranges, int max_ranges);
/* ... and the rows entry ("output rate per row"): out_rates [B], one launch; n_out [B] receives N_b, y is [B][S_out] with
 * S_out = max_b N_b (y_elems >= B * S_out), every column written. */
int vits_test_resample_rows(int device_id, const float *x, const int64_t *lens, int B, int S, int in_rate,
                            const int32_t *out_rates, float *y, size_t y_elems, int64_t *n_out);
/* The time warp by value ("intonation"): x [B][S] host, counts [B] the rows' valid samples (clipped to [0, S]), the rows'
 * segment records - row b's are segs[seg_first[b] .. seg_first[b + 1]) -, y [B][S_w] with S_w >= max(1, max_b N_b); every
 * column of y is written.  Records that do not continue their row (n0, pos0) or leave a token's limits are VITS_E_ARG. */
int vits_test_warp(int device_id, const float *x, const int64_t *counts, int B, int S, const vits_warp_seg *segs,
                   const int32_t *seg_first /* [B+1] */, float *y, int S_w);
/* ... and the glide ("pitch contours"): the same arguments over vits_glide_seg records, the pipeline's glide launch. */
int vits_test_glide(int device_id, const float *x, const int64_t *counts, int B, int S, const vits_glide_seg *segs,
                    const int32_t *seg_first /* [B+1] */, float *y, int S_w);
/* ... and both cut into pieces ("streamed pitch"): the input arrives in n_pieces pieces that end at piece_bounds[i] (ascending,
 * the last one S) and goes through the pipeline's stage - history, emit rule, windowed launches - on the pipeline's walk of a
 * poisoned buffer, with n_cap = vits_warp_stream_cap(longest piece, S_w).  S_w is exactly max(1, max_b N_b).  y [B][S_w]
 * receives the windows joined; ranges (nullable) [max_ranges][2] {first, n} of every window, in order.  Returns their number. */
int vits_test_warp_pieces(int device_id, const float *x, const int64_t *counts, int B, int S, const vits_warp_seg *segs,
                          const int32_t *seg_first /* [B+1] */, const int64_t *piece_bounds, int n_pieces, float *y, int S_w,
                          int64_t *ranges, int max_ranges);
int vits_test_glide_pieces(int device_id, const float *x, const int64_t *counts, int B, int S, const vits_glide_seg *segs,
                           const int32_t *seg_first /* [B+1] */, const int64_t *piece_bounds, int n_pieces, float *y, int S_w,
                           int64_t *ranges, int max_ranges);
/* The wide kernels by value ("pitch at an output rate"): x [B][S] host, row b at in_rates[b], counts [B], the rows' records within the
 * FOLDED limits (steps in [ONE / 8, 8 ONE], Kh <= 151, a gliding token at most 2^22 samples; vits_test_warp / vits_test_glide
 * keep refusing records outside the unfolded ones), out_rates [B] the rate each row is delivered at (0 or in_rates[b]: native).
 * A row without a record is an identity row: ceil(n_b * L / M) samples by the resampler's rule.  The launch renders output
 * samples [n_lo, n_hi) of every row into y [B][n_hi - n_lo]; every column is written, zeros behind N_b. */
int vits_test_warp_rate(int device_id, const float *x, const int64_t *counts, int B, int S, const vits_warp_seg *segs,
                        const int32_t *seg_first /* [B+1] */, const int32_t *in_rates, const int32_t *out_rates, int n_lo, int n_hi,
                        float *y);
int vits_test_glide_rate(int device_id, const float *x, const int64_t *counts, int B, int S, const vits_glide_seg *segs,
                         const int32_t *seg_first /* [B+1] */, const int32_t *in_rates, const int32_t *out_rates, int n_lo, int n_hi,
                        float *y);

/* ... and the wide streamed stage: vits_test_warp_pieces' walk over a folded plan at one pair of rates - what a chunked run
 * has - with n_cap = vits_warp_stream_cap_rate(longest piece, S_w, the plan's least step, its largest Kh). */
int vits_test_warp_rate_pieces(int device_id, const float *x, const int64_t *counts, int B, int S, const vits_warp_seg *segs,
                               const int32_t *seg_first /* [B+1] */, int in_rate, int out_rate, const int64_t *piece_bounds,
                               int n_pieces, float *y, int S_w, int64_t *ranges, int max_ranges);
int vits_test_glide_rate_pieces(int device_id, const float *x, const int64_t *counts, int B, int S, const vits_glide_seg *segs,
                                const int32_t *seg_first /* [B+1] */, int in_rate, int out_rate, const int64_t *piece_bounds,
                                int n_pieces, float *y, int S_w, int64_t *ranges, int max_ranges);

/* The kernels that turn tokens into frames and frames into samples, by value.  Every hook checks its sizes and extents on the
 * host (VITS_E_ARG) and launches the pipeline's kernel with the pipeline's grid.
 * Durations: logw [B][T] (the free form: w_ceil = ceil(exp(logw) * mask * length_scale [* token_rate]), length_scale the
 * utterance's column 1 of rows [B][3] when rows is given) or dur int64 [B][T] (the forced form), exactly one of them;
 * lens [B] within [0, T].  Out: w_ceil [B][T], cum int32 [B][T] (inclusive running sum), y_len int32 [B] (max(sum, 1)). */
int vits_test_durations(int device_id, const float *logw, const int64_t *dur, const int64_t *lens, int B, int T, float length_scale,
                        const float *rows, const float *token_rate, float *w_ceil, int32_t *cum, int32_t *y_len);
/* The fit kernel ("fitted durations") over weights w [B][T]: w_ceil / cum / y_len come in holding what the caller wants
 * rows of no group to keep (they are uploaded, the kernel runs, they are downloaded), scale / frames / status [n_groups]. */
int vits_test_fit_durations(int device_id, const float *w, const int64_t *lens, int B, int T, const vits_fit *fit, float *w_ceil,
                            int32_t *cum, int32_t *y_len, double *scale, int64_t *frames, int32_t *status);
/* Length regulator and prior sample: m_logs [B][2C][T] (m_p in the first C channels, logs_p in the second), cum / y_len as
 * vits_test_durations leaves them (y_len[b] <= F), noise (nullable) [B][C][noise_stride] of which the first noise_frames
 * <= noise_stride frames are read (zeros behind), else seeds (nullable) uint64 [B]: stream 2 of each utterance; noise_scale
 * or column 0 of rows [B][3].  Out: z_p [B][C][F]. */
int vits_test_expand_prior(int device_id, const float *m_logs, int B, int C, int T, const int32_t *cum, const int64_t *lens,
                           const int32_t *y_len, int F, const float *noise, int64_t noise_stride, int noise_frames,
                           float noise_scale, const float *rows, const uint64_t *seeds, float *z_p);
/* The flat noise stream (out [n]) and the per-utterance one (out [B][channels][T] = stream `stream` of seeds[b] times
 * rows[b][col], +0.0 where that is 0). */
int vits_test_fill_normal(int device_id, int64_t n, uint64_t seed, uint64_t stream_id, float *out);
int vits_test_fill_normal_rows(int device_id, int B, int channels, int T, const uint64_t *seeds, uint32_t stream, const float *rows,
                               int col, float *out);
/* The vocoder's tail, out [B][T] = tanh(conv_post(leaky_relu(x, slope))) with w [C][K], zeros at and behind vlen[b] * hop
 * (vlen nullable).  kernel 0: x planar [B][C][T]; 1: x in the raw layout [B][C/8][T][8], the 7-tap instantiation when K == 7;
 * 2: the same layout, always the generic instantiation.  C % 8 == 0 for 1 and 2; the staged tile must fit 64 KiB of LDS. */
int vits_test_post_conv(int device_id, const float *x, int B, int C, int T, const float *w, int K, float slope, const int64_t *vlen,
                        int hop, int kernel, float *out);

/* The text-side kernels of the encoder and the stochastic duration predictor, by value: LayerNorm, the DDSConv layers,
 * ConvFlow.pre, the inverse spline and the ElementwiseAffine.  The hooks launch through the pipeline's own launch functions;
 * the form is an ARGUMENT (the VITSMI_* switches are read once per process and select nothing here).  Every `out` holds a
 * guard row of T elements behind the tensor (T cells of 8 for planes): outputs are pre-filled with 0xff bytes, so an element
 * never written and a write past the end both show.  Argument combinations the pipeline never forms are VITS_E_ARG.
 * LayerNorm over channels of x [B][C][T]: flags = 1 GELU | 2 ACCUM (out += ...) | 4 MASK (lens) | 8 RELU_IN; form 0 = 16 time
 * steps per workgroup, 1 = 32 (both C <= 256), 2 = one lane per column (any C); out_init (nullable) = the initial content of
 * out; in_place: x is the initial content of out and the kernel reads it there.  dw_w [C][K] (nullable) with dw_b, K, dil: the
 * depthwise conv of x * mask in front of LN + GELU (flags = 1, out of place, form 1 for C <= 256 and 2 above).  planes
 * (nullable, tile forms, C % 8 == 0): the result's fp16 operand planes [B][3][C/8][T][8] (the third plane is not written).
 * out: B * C * T + T floats; planes: B * 3 * C * T + 8 T halves. */
int vits_test_layernorm(int device_id, const float *x, const float *out_init, int B, int C, int T, const float *gamma,
                        const float *beta, const int64_t *lens, int flags, int form, int in_place, const float *dw_w,
                        const float *dw_b, int K, int dil, float *out, uint16_t *planes);
/* A stack of n_layers <= 4 fused DDSConv layers (k = 3) on x [B][C][T]: form 16 = dds_layer16_kernel (C in 64, 128, 192, 256),
 * 32 = dds_layer_kernel (32, 64, 96, 128, 192, 256).  mask_out 1: the stack as the pipeline runs it (buffer ping-pong, mask
 * behind the last layer), the result read where the pipeline reads it; 0: ONE layer launched with its mask off.
 * Head (form 16, n_layers >= 2; head_cond nullable): the stack's input is head_w[c] * z[b][head_ch][t] + head_b[c] +
 * head_cond[b][c][t] with z [B][2][T]; x is then not read.  Tail (form 16; tail_w [tail_rows][C] nullable, tail_b nullable,
 * tail_rows <= C): out = (tail_w . result + tail_b) * mask, [B][tail_rows][T].  out: B * (C or tail_rows) * T + T floats. */
typedef struct vits_test_dds_layer {
    const float *dw_w, *dw_b;   /* depthwise [C][3], [C] */
    const float *ln1_g, *ln1_b; /* [C] */
    const float *pw_w, *pw_b;   /* 1 x 1 conv [C][C], [C] */
    const float *ln2_g, *ln2_b; /* [C] */
    int32_t dil;
} vits_test_dds_layer;
int vits_test_dds(int device_id, int form, const float *x, int B, int C, int T, const int64_t *lens, int n_layers,
                  const vits_test_dds_layer *layers, int mask_out, const float *head_cond, const float *head_z, int head_ch,
                  const float *head_w, const float *head_b, const float *tail_w, const float *tail_b, int tail_rows, float *out);
/* ConvFlow.pre + conditioning: out[b][c][t] = w[c] * z[b][ch][t] + bias[c] + cond[b][c][t]; z [B][2][T].  out: B * C * T + T. */
int vits_test_cf_pre(int device_id, const float *z, int ch, const float *w, const float *bias, const float *cond, int B, int C, int T,
                     float *out);
/* The inverse rational-quadratic spline with linear tails (tail bound 5) on z [B][2][T]: channel ch0 passes through, channel
 * ch0 ^ 1 is transformed with pr [B][3 nb - 1][T] (widths, heights: divided by sqrt_c; derivatives), both masked by lens.
 * nb <= 10 runs rqs_inverse_kernel<10>, up to 16 <16>.  out: B * 2 * T + T. */
int vits_test_rqs_inverse(int device_id, const float *pr, const float *z, int B, int T, const int64_t *lens, int ch0, int nb,
                          float sqrt_c, float *out);
/* ElementwiseAffine reverse on channel ch of z [B][2][T]: out[b][t] = (z - m0) * exp(-logs0) * mask.  out: B * T + T. */
int vits_test_ea_logw(int device_id, const float *z, int ch, float m0, float logs0, const int64_t *lens, int B, int T, float *out);

/* The delivery by value: x [B][S] host, counts [B] the rows' valid samples (within [0, S]; what lies behind must not show);
 * launches the pipeline's kernels with the pipeline's grids.  Everything else as vits_deliver. */
int vits_test_deliver(int device_id, const float *x, const int64_t *counts, int B, int S, const vits_segment *segs, int n_segs,
                      int n_streams, int encoding, void *dst, size_t dst_bytes, int64_t *stream_samples, int64_t *stream_offsets);

/* The trimmed delivery by value: x, counts as vits_test_deliver; launches the pipeline's kernels with the pipeline's grids.
 * Everything else as vits_deliver_trimmed. */
int vits_test_deliver_trimmed(int device_id, const float *x, const int64_t *counts, int B, int S, const vits_segment *segs,
                              const vits_trim *trims, int n_segs, int n_streams, int encoding, void *dst, size_t dst_bytes,
                              int64_t *stream_samples, int64_t *stream_offsets, int64_t *kept_first, int64_t *kept_count);

/* The loudness kernels by value: x [B][S] host, row b's kept range x[b][firsts[b] .. firsts[b] + counts[b]) (within the row;
 * what lies outside must not show), all rows in one set of launches with the pipeline's grids.  n_sub [B] receives every
 * row's whole sub-blocks, e their energies back to back (e_cap >= their sum, else VITS_E_ARG), *chunk the compiled Lc. */
int vits_test_loudness_blocks(int device_id, const float *x, const int64_t *counts, const int64_t *firsts, int B, int S,
                              int sample_rate, float *e, size_t e_cap, int32_t *n_sub, int32_t *chunk);

/* The levelled delivery by value: as vits_test_deliver_trimmed; everything else as vits_deliver_leveled. */
int vits_test_deliver_leveled(int device_id, const float *x, const int64_t *counts, int B, int S, const vits_segment *segs,
                              const vits_trim *trims, const vits_level *levels, int n_segs, int n_streams, int encoding,
                              int sample_rate, void *dst, size_t dst_bytes, int64_t *stream_samples, int64_t *stream_offsets,
                              int64_t *kept_first, int64_t *kept_count, double *loudness, float *gain);

/* The shaped delivery by value: as vits_test_deliver_leveled; everything else as vits_deliver_shaped. */
int vits_test_deliver_shaped(int device_id, const float *x, const int64_t *counts, int B, int S, const vits_segment *segs,
                             const vits_trim *trims, const vits_level *levels, const vits_shape *shapes, const vits_env_point *points,
                             int64_t n_points, int n_segs, int n_streams, int encoding, int sample_rate, void *dst, size_t dst_bytes,
                             int64_t *stream_samples, int64_t *stream_offsets, int64_t *kept_first, int64_t *kept_count,
                             double *loudness, float *gain);

/* The limited delivery by value: as vits_test_deliver_shaped; everything else as vits_deliver_limited. */
int vits_test_deliver_limited(int device_id, const float *x, const int64_t *counts, int B, int S, const vits_segment *segs,
                              const vits_trim *trims, const vits_level *levels, const vits_shape *shapes, const vits_env_point *points,
                              int64_t n_points, const vits_limit *limits, int n_segs, int n_streams, int encoding, int sample_rate,
                              void *dst, size_t dst_bytes, int64_t *stream_samples, int64_t *stream_offsets, int64_t *kept_first,
                              int64_t *kept_count, double *loudness, float *gain);

/* The encoded stream's kernel by value: x [B][S] host, counts [B] the rows' valid samples (within [0, S]; what lies behind
 * must not show).  Columns [0, S) are cut into pieces of piece_samples samples (the last one shorter); each piece goes through
 * the pipeline's kernel with the pipeline's grid.  The pieces' [B][pitch] blocks land back to back in bytes (bytes_cap >= their
 * sum); pitches [piece], valid [piece][B] and peaks [piece][B] are per piece (max_pieces of each).  Returns the number of
 * pieces. */
int vits_test_stream_pack(int device_id, const float *x, const int64_t *counts, int B, int S, int piece_samples,
                          const vits_stream_format *fmt, void *bytes, size_t bytes_cap, int64_t *pitches, int32_t *valid,
                          float *peaks, int max_pieces);

/* vits_test_stream_pack with a shaping (nullable; its plan is not called).  Every piece goes through the pipeline's kernels -
 * the shaped one, or the limited one and the carry - and delivers the range of vits_stream_emit_range: firsts [piece] and
 * ns [piece] receive it.  A piece that delivers nothing has n 0 and pitch 0, lands no bytes and leaves its valid and peaks
 * untouched.  Returns the number of pieces. */
int vits_test_stream_pack_shaped(int device_id, const float *x, const int64_t *counts, int B, int S, int piece_samples,
                                 const vits_stream_format *fmt, const vits_stream_shaping *shaping, void *bytes, size_t bytes_cap,
                                 int64_t *pitches, int32_t *valid, float *peaks, int64_t *firsts, int64_t *ns, int max_pieces);

/* vits_test_stream_pack_shaped with onsets (nullable): every piece goes through the scan and the pipeline's kernels.
 * skip [piece][B] as valid; start [B] receives the rows' final a_b (INT32_MAX where a trimmed row has no onset, 0 for a row
 * that is not trimmed).  Returns the number of pieces. */
int vits_test_stream_pack_trimmed(int device_id, const float *x, const int64_t *counts, int B, int S, int piece_samples,
                                  const vits_stream_format *fmt, const vits_stream_shaping *shaping, const vits_stream_onset *onsets,
                                  void *bytes, size_t bytes_cap, int64_t *pitches, int32_t *valid, int32_t *skip, float *peaks,
                                  int64_t *firsts, int64_t *ns, int32_t *start, int max_pieces);

#ifdef __cplusplus
}
#endif
#endif /* VITSMI_H */
