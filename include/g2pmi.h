/*
 * g2pmi.h — C ABI of the ByT5 G2P engine inside libvitsmi.so: the byte-level T5 encoder-decoder that
 * phoonnx's multilingual phonemizer runs through onnxruntime, as hand-written gfx950 kernels.
 *
 * Reference interface replaced (paths relative to the phoonnx checkout):
 *   - session construction      phoonnx/phonemizers/mul.py:106      -> g2p_open()
 *   - session.get_outputs()     phoonnx/phonemizers/mul.py:183      -> g2p_output_name()
 *   - session.run(names, feed)  phoonnx/phonemizers/mul.py:199-211  -> g2p_run()   (logits of every decoder position)
 *   - the greedy loop around it phoonnx/phonemizers/mul.py:192-230  -> g2p_generate() (one call, KV cache, on the device:
 *     the reference re-runs the whole graph, encoder included, for every generated token)
 * The graph is Hugging Face transformers' T5ForConditionalGeneration exported to ONNX (inputs input_ids, attention_mask,
 * decoder_input_ids; output logits); weights are read from the same .onnx file.
 *
 * Conventions as in vitsmi.h: plain pointers and sizes; int functions return 0 or a negative VITS_E_* code
 * (vitsmi.h), message from g2p_last_error().  g2p_run: batch size 1, as the reference calls it.
 */
#ifndef G2PMI_H
#define G2PMI_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct g2p_handle g2p_handle;

/* Parse `onnx_path`, derive the model description (d_model, heads, layers, feed-forward type ... from shapes and node
 * names), pack the weights on GPU `device_id`.  device_id < 0: host-only handle (description only; g2p_run fails). */
int g2p_open(const char *onnx_path, int device_id, g2p_handle **out);
void g2p_close(g2p_handle *h);
const char *g2p_last_error(g2p_handle *h);

/* "vocab","d_model","heads","d_kv","d_ff","n_enc","n_dec","num_buckets","max_distance","gated","act","scale_out" */
int g2p_hparam(g2p_handle *h, const char *key, int64_t *out);
int g2p_num_outputs(g2p_handle *h);
const char *g2p_output_name(g2p_handle *h, int i);  /* "logits" */

/* Relative-position bucket of (key position - query position) = rel, as the graph computes it (an integer: exact).
 * decoder != 0: the causal variant. */
int g2p_bucket(g2p_handle *h, int decoder, int rel);

/* What session.run returns (mul.py:210-211): logits [1, T, vocab] (host float32, T * vocab values) for
 * input_ids [1, S] and decoder_input_ids [1, T].  attention_mask may be NULL (all ones, what mul.py:187 builds) or
 * right-padded (ones, then zeros: the padded positions are dropped, which is what masking them amounts to); a mask
 * with holes is rejected. */
int g2p_run(g2p_handle *h, const int64_t *input_ids, int S, const int64_t *attention_mask, const int64_t *decoder_input_ids,
            int T, float *logits);

/* The greedy loop of mul.py:192-230 in one call: encoder once, then one decoder step per token with a key/value cache,
 * argmax on the device; stops at eos_id (included in the output, as the reference appends it before breaking) or after
 * max_length tokens.  out_ids receives at most max_length ids; *n_out their count. */
int g2p_generate(g2p_handle *h, const int64_t *input_ids, int S, int max_length, int64_t start_id, int64_t eos_id,
                 int64_t *out_ids, int *n_out);

/* The same loop for B independent inputs side by side (extension: the reference phonemizes chunk after chunk,
 * base.py:66-70): input_ids holds the B sequences back to back, lens[b] their lengths.  One encoder pass over the padded
 * batch (padding is masked out of every attention), then every decoder step streams the weights once for all B
 * sequences; a sequence that has produced eos_id stops collecting tokens while the others finish.  Each sequence's ids
 * are exactly what g2p_generate returns for it alone.  out_ids: [B][max_length]; n_out: [B].  B <= G2P_MAX_BATCH. */
#define G2P_MAX_BATCH 64
int g2p_generate_batch(g2p_handle *h, const int64_t *input_ids, const int *lens, int B, int max_length, int64_t start_id,
                       int64_t eos_id, int64_t *out_ids, int *n_out);

/* Test hook (not part of the product surface): the decoder-STEP path (the kernels g2p_generate_batch runs per token) with
 * GIVEN decoder inputs instead of its own argmax fed back, returning the logits of every step: logits[b][t] = what g2p_run
 * returns at position t for decoder_input_ids[b][0 .. t].  B <= G2P_MAX_BATCH inputs back to back in input_ids (lens[b]
 * each), decoder_input_ids [B][T] (column 0 = the start token), logits [B][T][vocab].  B <= 4 runs the matrix-vector step
 * (NB = 1 / 2 / 4, one-query attention over the key / value caches); B > 4 the wide step (sequences as the columns of
 * [C][NB] activations, NB = B rounded up to 8: the short-sequence linear kernels writing into the caches).  The greedy ids
 * of a randomly initialised model are nearly constant sequences; this compares the step path number by number. */
int g2p_test_forced_steps(g2p_handle *h, const int64_t *input_ids, const int *lens, int B, const int64_t *decoder_input_ids, int T,
                          float *logits);

/* Test hook: the short-sequence Linear launch of the engine on host buffers, through the engine's own choice of kernel.
 * y[j][row * y_rs + col * y_cs] = sum_k W[j][row][k] x[k][col] (+ res[j][same place]) for njobs (1 .. 3) matrices
 * W[j] [out[j]][in] over one x [in][T] (pitch xp >= T).  res may be NULL, and so may its entries.  y[j] and res[j] hold
 * (out[j] - 1) * y_rs + (T - 1) * y_cs + 1 floats; what the kernel does not write comes back unchanged.  The strides must
 * give every (row, column) an element of its own.  mode 0: the kernel the engine would choose; 1: the generic kernel. */
int g2p_test_linear(int device, int njobs, const float *const *W, const int *out, int in, const float *x, int T, int xp,
                    const float *const *res, int64_t y_rs, int64_t y_cs, int mode, float *const *y);

/* Test hook: the decoder step's matrix-vector launch for NB (1, 2 or 4) sequences, njobs (1 .. 3) matrices:
 * y[j][b][row] = post * rs_b * sum_i W[j][row][i] g[i] x[b][i], rs_b = rsqrt(mean(x[b]^2) + eps) if g else 1 (g NULL: g[i] = 1);
 * with W2[j]: y = act(that) * (the same with W2[j]); without: act applied if act >= 0 (0 gelu_new, 1 relu, 2 gelu erf);
 * + res[j][b][row] if given.  x [NB][in], y[j] / res[j] [NB][out[j]]. */
int g2p_test_step(int device, int NB, int njobs, const float *const *W, const float *const *W2, const int *out, int in,
                  const float *x, const float *g, int act, float eps, float post, const float *const *res, float *const *y);

/* Test hook: one launch of the attention kernel, as the engine launches it, on host buffers.  Query / output element
 * (channel ch of heads * dk, column c of cols) at ch * q_cs + c * q_ts; q and out hold (heads * dk - 1) * q_cs + (cols - 1) * q_ts
 * + 1 floats, and out comes back with everything the kernel does not write unchanged.  Column c is query i = c % seg of
 * sequence b = c / seg, at position i + q_off; its keys / values (kv_n floats each) start b * kv_bs floats into k / v, channel
 * stride kp, and number lens[b] (lens NULL: Tk), of which a causal launch takes those at positions <= i + q_off.
 * score_j = q . k_j + bias[lut[j - (i + q_off) + max_positions - 1]][head]: bias [num_buckets][heads], lut 2 * max_positions - 1
 * buckets, both NULL for no bias.  Refused: Tk outside [1, max_positions), lens outside [1, Tk], cols not whole sequences,
 * a lut index or a bucket outside its table, q / out strides that make two elements one, k / v too short. */
int g2p_test_attention(int device, const float *q, float *out, int q_cs, int q_ts, const float *k, const float *v, int64_t kv_n,
                       int kp, int64_t kv_bs, const float *bias, int num_buckets, const int *lut, int heads, int dk, int cols, int seg,
                       const int *lens, int Tk, int q_off, int causal);

/* Test hook: the RMS-norm kernel.  y[c][t] = x[c][t] * rsqrt(mean_c(x[.][t]^2) + eps) * g[c] for t < T; x [C][xpitch], y [C][ypitch]
 * (in and out: columns T .. ypitch - 1 come back unchanged). */
int g2p_test_rmsnorm(int device, const float *x, const float *g, float *y, int C, int T, int xpitch, int ypitch, float eps);

/* Test hook: the argmax kernel for NB sequences.  Logit v of sequence b at logits[b * lb + v * pitch + t] (the wide step:
 * pitch NB, lb 1; the narrow one: pitch 1, lb V); the first maximum goes to ids[b * ib + slot] and to the same place of host_copy
 * (both [NB][ib], in and out). */
int g2p_test_argmax(int device, const float *logits, int V, int pitch, int t, int64_t lb, int NB, int64_t *ids, int64_t *host_copy,
                    int64_t ib, int slot);

#ifdef __cplusplus
}
#endif
#endif /* G2PMI_H */
