// g2p_workspace.hpp — the device workspace of the two G2P runs, each stated once as the walk that carves it (slab.hpp):
// measured by a dry walk, reserved, then carved by the same call.  Host-side C++17, no HIP types.
#pragma once
#include <cstdint>
#include <vector>

#include "g2p_model.hpp"
#include "slab.hpp"

namespace vitsmi {

// g2p_run: S input ids, T decoder positions (teacher forced)
struct G2PRunBufs {
    int64_t *in, *dec;
    float *xe, *xd, *hn, *q, *k, *v, *att;  // activations [max(d_model, inner)][max(S, T)]
    float *fa, *fb;                         // feed-forward hidden [d_ff][max(S, T)]
    float *kc, *vc;                         // cross-attention keys / values [inner][S]
    float *lg, *lgt;                        // logits [vocab][T] and their transpose
};

inline G2PRunBufs carve_g2p_run(Carver &cv, const G2PModel &m, int S, int T) {
    G2PRunBufs w{};
    const int L = S > T ? S : T;
    const size_t nA = (size_t)(m.d_model > m.inner ? m.d_model : m.inner) * L;
    w.in = cv.take<int64_t>(S);
    w.dec = cv.take<int64_t>(T);
    for (float **p : {&w.xe, &w.xd, &w.hn, &w.q, &w.k, &w.v, &w.att}) *p = cv.take<float>(nA);
    w.fa = cv.take<float>((size_t)m.d_ff * L);
    w.fb = cv.take<float>((size_t)m.d_ff * L);
    w.kc = cv.take<float>((size_t)m.inner * S);
    w.vc = cv.take<float>((size_t)m.inner * S);
    w.lg = cv.take<float>((size_t)m.vocab * T);
    w.lgt = cv.take<float>((size_t)m.vocab * T);
    return w;
}

// the persistent step's grid barrier: top counter + give-up flag, then a line per group
constexpr size_t kG2PBarrierWords = 32 * (1 + 4096 / 4);

// g2p_generate: NB sequences of S input ids side by side, TM decoder positions each.  `forced` (the decoder inputs are given,
// every step's logits kept) and `persist` (the narrow step as one persistent launch over a table of Phase records) are
// the run's own arguments.
template <class Phase>
struct G2PGenerateBufs {
    int64_t *in, *gen;
    int *lens;
    float *xe, *hn, *q, *k, *v, *att;  // encoder activations [max(d_model, inner)][NB * S]
    float *fa, *fb;                    // feed-forward hidden [d_ff][NB * S]
    // per decoder layer: self-attention cache [NB][inner][TM]; cross-attention keys / values of the encoder output [inner][NB * S]
    std::vector<float *> ks, vs, kc, vc;
    float *x1, *q1, *a1, *f1, *lg;  // one step's activations
    float *h1, *f2;                 // (wide step only)
    int64_t *arg;    // forced: the argmax lands in a scratch copy of the id table (the given inputs stay); else `gen`
    float *steplog;  // forced: every step's logits [TM - 1][NB][vocab]
    Phase *ph;       // persist: the step's 3 + 8 * layers phases
    unsigned *bar;   // persist: kG2PBarrierWords
};

template <class Phase>
G2PGenerateBufs<Phase> carve_g2p_generate(Carver &cv, const G2PModel &m, int S, int NB, int TM, bool forced, bool persist) {
    G2PGenerateBufs<Phase> w{};
    const size_t T = (size_t)S * NB, nA = (size_t)(m.d_model > m.inner ? m.d_model : m.inner) * T;
    w.in = cv.take<int64_t>(T);
    w.gen = cv.take<int64_t>((size_t)NB * TM);
    w.lens = cv.take<int>(NB);
    for (float **p : {&w.xe, &w.hn, &w.q, &w.k, &w.v, &w.att}) *p = cv.take<float>(nA);
    w.fa = cv.take<float>((size_t)m.d_ff * T);
    w.fb = cv.take<float>((size_t)m.d_ff * T);
    for (size_t l = 0; l < m.dec.size(); l++) {
        w.ks.push_back(cv.take<float>((size_t)NB * m.inner * TM));
        w.vs.push_back(cv.take<float>((size_t)NB * m.inner * TM));
        w.kc.push_back(cv.take<float>((size_t)m.inner * T));
        w.vc.push_back(cv.take<float>((size_t)m.inner * T));
    }
    w.x1 = cv.take<float>((size_t)NB * m.d_model);
    w.q1 = cv.take<float>((size_t)NB * m.inner);
    w.a1 = cv.take<float>((size_t)NB * m.inner);
    w.f1 = cv.take<float>((size_t)NB * m.d_ff);
    w.lg = cv.take<float>((size_t)NB * m.vocab);
    w.h1 = cv.take<float>((size_t)NB * m.d_model);
    w.f2 = cv.take<float>((size_t)NB * m.d_ff);
    w.arg = forced ? cv.take<int64_t>((size_t)NB * TM) : w.gen;
    if (forced) w.steplog = cv.take<float>((size_t)(TM - 1) * NB * m.vocab);
    if (persist) {
        w.ph = cv.take<Phase>(3 + 8 * m.dec.size());
        w.bar = cv.take<unsigned>(kG2PBarrierWords);
    }
    return w;
}

}  // namespace vitsmi
