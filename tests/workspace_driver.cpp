// Driver of test_workspace_cpu.py: model.cpp + onnx_reader.cpp + workspace.hpp + slab.hpp, no HIP.  Builds every voice given
// on the command line at every precision and walks each workspace plan over a grid of request sizes: once dry, once over a
// fake base (never dereferenced), once with one byte too little.  One line per (voice, precision, B, T, F, chunk):
//   <voice> <precision> <B> <T> <F> <chunk> A <tok> <frm> <voc> <io_in> <io_pcm>   bytes of each plan; every check held
//   <voice> <precision> <B> <T> <F> <chunk> V <what>                               a check failed
//   <voice> <precision> <B> <T> <F> <chunk> R <message>                            the packer refused the voice
// The extents below are what the kernels need of each buffer, written here independently of the walks.
#include <algorithm>
#include <cstdio>
#include <functional>
#include <string>
#include <vector>

#include "workspace.hpp"

using namespace vitsmi;

namespace {

struct Ext {
    const char *name;
    const void *p;
    size_t bytes;
};

char *const kBase = reinterpret_cast<char *>(uintptr_t(1) << 44);

// dry == real, alignment, no overlap at the stated extents, overflow reported at one byte less; returns "" or what failed
std::string check(const char *plan, const std::function<std::vector<Ext>(Carver &)> &walk, size_t *bytes) {
    Carver dry;
    for (const Ext &e : walk(dry))
        if (e.p) return std::string(plan) + ": a dry walk returned a pointer for " + e.name;
    *bytes = dry.used;
    Carver real(kBase, dry.used);
    std::vector<Ext> ex = walk(real);
    if (real.used != dry.used) return std::string(plan) + ": the real walk ends at " + std::to_string(real.used) + ", the dry one at " + std::to_string(dry.used);
    if (!real.fits()) return std::string(plan) + ": the real walk does not fit its own measure";
    std::sort(ex.begin(), ex.end(), [](const Ext &a, const Ext &b) { return a.p < b.p; });
    for (size_t i = 0; i < ex.size(); i++) {
        const char *p = static_cast<const char *>(ex[i].p);
        if (!p || p < kBase) return std::string(plan) + ": no pointer for " + ex[i].name;
        if ((p - kBase) % 256) return std::string(plan) + ": " + ex[i].name + " is not 256-byte aligned";
        const char *end = i + 1 < ex.size() ? static_cast<const char *>(ex[i + 1].p) : kBase + real.used;
        if (p + ex[i].bytes > end) return std::string(plan) + ": " + ex[i].name + " overlaps " + (i + 1 < ex.size() ? ex[i + 1].name : "the end");
    }
    if (dry.used > 0) {
        Carver tight(kBase, dry.used - 1);
        walk(tight);
        if (tight.fits()) return std::string(plan) + ": one byte less was not reported";
    }
    return "";
}

size_t planes(size_t n) { return (n * 3 / 2 + 64) * 4; }  // three 16-bit slots per element + 64 floats of whole-cell margin

std::vector<Ext> tokens(Carver &cv, const Model &m, int B, int T) {
    const TokenBufs t = carve_tokens(cv, m, B, T);
    const size_t nBT = (size_t)B * T, nHT = nBT * m.H;
    std::vector<Ext> e = {{"len", t.len, (size_t)B * 4}, {"ylen64", t.ylen64, (size_t)B * 8}, {"cum", t.cum, nBT * 4},
                          {"x", t.x, nHT * 4}, {"att", t.att, nHT * 4}, {"xe", t.xe, nHT * 4}, {"qkv", t.qkv, 3 * nHT * 4},
                          {"ffh", t.ffh, nBT * m.FF * 4}, {"stats", t.stats, nBT * 2 * m.C * 4}, {"logw", t.logw, nBT * 4},
                          {"wceil", t.wceil, (nBT + B) * 4}, {"rows", t.rows, (size_t)B * 12}, {"seeds", t.seeds, (size_t)B * 8},
                          {"ctl", t.ctl, nBT * 8}};
    if (m.enc_sx) {
        e.push_back({"x_pl", t.x_pl, planes(nHT)});
        e.push_back({"att_pl", t.att_pl, planes(nHT)});
        e.push_back({"ff_pl", t.ff_pl, planes(nBT * m.FF)});
        if (attention16_ok(m.dk, m.window)) e.push_back({"qkv_pl", t.qkv_pl, (nHT * 9 / 2 + 64) * 4});
    }
    if (m.gin) e.push_back({"dp_cond", t.dp_cond, (size_t)B * m.dp_cond_rows * 4});
    if (m.use_sdp) {
        const size_t n = nBT * m.dp_pre.Cout * 4;
        int bins = 0;
        for (const auto &cf : m.cf) bins = cf.proj.Cout > bins ? cf.proj.Cout : bins;
        for (const Ext &x : {Ext{"hb", t.hb, n}, Ext{"y", t.y, n}, Ext{"y2", t.y2, n}, Ext{"cond", t.cond, n}, Ext{"h2", t.h2, n},
                             Ext{"pr", t.pr, nBT * bins * 4}, Ext{"z", t.z, nBT * 8}})
            e.push_back(x);
    } else {
        if (m.gin) e.push_back({"xi", t.xi, nHT * 4});
        e.push_back({"h1", t.h1, nBT * m.dpp_F * 4});
        e.push_back({"h2", t.h2, nBT * m.dpp_F * 4});
    }
    return e;
}

// the generator rendering n frames (the largest tensor of any stage decides every region)
void generator(std::vector<Ext> &e, const GenBufs &g, const Model &m, int B, int n) {
    size_t R = (size_t)B * std::max(m.C0, m.C) * ((n + 3) & ~3);
    int64_t t = n;
    for (const auto &st : m.ups) R = std::max(R, (size_t)B * st.C * (size_t)(t *= st.u));
    e.push_back({"yl", g.yl, (size_t)B * 4});
    if (!m.gen_sx) {
        for (int i = 0; i < 10; i++) e.push_back({"reg", g.reg[i], R * 4});
        if (g.out != g.reg[9]) e.push_back({"out (not reg[9])", nullptr, 0});
        return;
    }
    for (const uint16_t *p : {g.stage_in[0], g.stage_in[1], g.y_pl, g.raa[0], g.raa[1], g.tmp_pl}) e.push_back({"planes", p, planes(R)});
    if (!m.gen_planes)
        for (const float *p : {g.y_raw, g.ra[0], g.ra[1]}) e.push_back({"raw", p, R * 4});
    e.push_back({"xs_raw", g.xs_raw, R * 4});
    e.push_back({"out", g.out, (size_t)B * n * m.hop * 4});
}

std::vector<Ext> frames(Carver &cv, const Model &m, int B, int F, int chunk, bool flow) {
    const int Fgen = gen_frames(m, F, chunk);
    const FrameBufs f = carve_frames(cv, m, B, F, Fgen, flow);
    const size_t nCF = (size_t)B * m.C * F * 4, nHF = (size_t)B * m.flow_H * F * 4;
    std::vector<Ext> e;
    if (flow) {
        const FlowBufs &w = f.flow;
        // (hx_pl: up to three 16-bit planes of [B][flow_H][F]; skip_pl: two; x0_pl: two of one half of [B][C][F])
        e = {{"zp", w.zp, nCF}, {"z", w.z, nCF}, {"g", w.g, nCF}, {"hx", w.hx, nHF}, {"skip", w.skip, nHF}, {"acts", w.acts, nHF},
             {"a2", w.a2, 2 * nHF}, {"hx_pl", w.hx_pl, nHF * 3 / 2}, {"x0_pl", w.x0_pl, nCF / 2}, {"skip_pl", w.skip_pl, nHF}};
        if (m.gin) {
            if (w.gc.size() != m.flow.size()) e.push_back({"gc (one per coupling)", nullptr, 0});
            for (size_t i = 0; i < w.gc.size(); i++) e.push_back({"gc", w.gc[i], (size_t)B * 2 * m.flow_H * m.flow[i].n_wn * 4});
            e.push_back({"dec_cond", w.dec_cond, (size_t)B * m.C0 * 4});
        }
    } else {
        e = {{"z", f.voc.z, nCF}};
        if (m.gin) {
            e.push_back({"sid", f.voc.sid, (size_t)B * 8});
            e.push_back({"dec_cond", f.voc.dec_cond, (size_t)B * m.C0 * 4});
        }
    }
    if (cv.base && (const char *)f.gen.yl != cv.base + ((f.gen_at + 255) & ~size_t(255)))
        e.push_back({"gen_at (the mark in front of the generator's first buffer)", nullptr, 0});
    generator(e, f.gen, m, B, Fgen);
    // a chunk carves the generator's part again: same call, same buffers
    const size_t end = cv.used;
    cv.rewind(f.gen_at);
    const GenBufs again = carve_generator(cv, m, B, Fgen);
    if (cv.used != end || again.yl != f.gen.yl || again.out != f.gen.out || again.xs_raw != f.gen.xs_raw || again.reg[0] != f.gen.reg[0])
        e.push_back({"generator (carved again after rewind)", nullptr, 0});
    return e;
}

std::vector<Ext> inputs(Carver &cv, const Model &m, int B, int T, int Fz) {
    const InputBufs i = carve_inputs(cv, m, B, T, T, Fz);
    if (cv.base && (i.lens != i.ids + (size_t)B * T || i.sid != i.lens + B)) return {{"ids | lens | sid (contiguous)", nullptr, 0}};
    return {{"ids|lens|sid", i.ids, ((size_t)B * T + 2 * (size_t)B) * 8}, {"noise_dp", i.noise_dp, (size_t)B * 2 * T * 4},
            {"noise_z", i.noise_z, (size_t)B * m.C * Fz * 4}};
}

std::vector<Ext> pcm16(Carver &cv, int B, size_t S) {
    const PcmBufs p = carve_pcm16(cv, B, (int)S);
    return {{"pcm", p.pcm, (size_t)B * S * 2}, {"peak", p.peak, (size_t)B * 4}};
}

}  // namespace

int main(int argc, char **argv) {
    const int Bs[] = {1, 2, 8, 32, 256}, Ts[] = {1, 4, 37, 256, 1024}, Fs[] = {1, 4, 63, 1000, 8000}, chunks[] = {0, 16, 64};
    for (int a = 1; a < argc; a++) {
        std::string voice = argv[a];
        voice = voice.substr(voice.find_last_of('/') + 1);
        OnnxModel om;
        std::string err = om.load(argv[a]);
        for (const char *prec : {"f16x3", "bf16x6", "f16"}) {
            Model m;
            std::string refused = err.empty() ? m.build(om, /*layout_only=*/false, prec) : err;
            for (int B : Bs)
                for (int T : Ts)
                    for (int F : Fs)
                        for (int chunk : chunks) {
                            printf("%s %s %d %d %d %d ", voice.c_str(), prec, B, T, F, chunk);
                            if (!refused.empty()) {
                                printf("R %s\n", refused.c_str());
                                continue;
                            }
                            const int Fp = (F + 3) & ~3;  // the flow runs on whole groups of 4 frames
                            size_t tok = 0, frm = 0, voc = 0, in = 0, pcm = 0;
                            std::string v = check("tokens", [&](Carver &cv) { return tokens(cv, m, B, T); }, &tok);
                            if (v.empty()) v = check("frames", [&](Carver &cv) { return frames(cv, m, B, Fp, chunk, true); }, &frm);
                            if (v.empty()) v = check("vocoder", [&](Carver &cv) { return frames(cv, m, B, F, chunk, false); }, &voc);
                            if (v.empty()) v = check("inputs", [&](Carver &cv) { return inputs(cv, m, B, T, Fp); }, &in);
                            if (v.empty()) v = check("pcm16", [&](Carver &cv) { return pcm16(cv, B, (size_t)F * m.hop); }, &pcm);
                            if (v.empty()) printf("A %zu %zu %zu %zu %zu\n", tok, frm, voc, in, pcm);
                            else printf("V %s\n", v.c_str());
                        }
        }
    }
    return 0;
}
