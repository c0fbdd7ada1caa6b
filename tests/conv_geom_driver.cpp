// Driver of test_conv_geom_cpu.py: model.cpp + onnx_reader.cpp + conv_geom.hpp, no HIP.  Packs every conv of the boundary
// grid in every format and asks the shared stage functions (the ones the launchers take their geometry and refusals from)
// about each packing that was accepted: its own tile and every tile conv_sx() may run it on.  One line per row:
//   <format> <Cin> <Cout> <K> <dil|stride> A            accepted, and launchable
//   <format> <Cin> <Cout> <K> <dil|stride> V <what>     accepted, but a launcher would refuse it
//   <format> <Cin> <Cout> <K> <dil|stride> R <message>  refused
#include <atomic>
#include <cstdio>
#include <string>
#include <thread>
#include <vector>

#include "conv_geom.hpp"
#include "model.hpp"

using namespace vitsmi;

namespace {

struct Format {
    const char *name;
    int hint;  // 0-2: f32 engine size class, 3: sx engine
    TestPack o;
};

std::vector<Format> formats() {
    std::vector<Format> f = {{"f32_hint0", 0, {}}, {"f32_hint1", 1, {}}, {"f32_hint2", 2, {}}};
    auto sx = [&](const char *n, SxPack::Planes p, bool force16, bool no_s16) {
        TestPack o;
        o.sx.planes = p;
        o.sx.force16 = force16;
        o.sx.no_s16 = no_s16;
        f.push_back({n, 3, o});
    };
    sx("sx_bf16x3", SxPack::BF16X3, false, false);
    sx("sx_f16x2", SxPack::F16X2, false, false);
    sx("sx_f16x1", SxPack::F16X1, false, false);
    sx("sx_f16x2_force16", SxPack::F16X2, true, false);
    sx("sx_f16x2_no_s16", SxPack::F16X2, false, true);
    return f;
}

// "" when every launch of this packing finds its stage, else what would be refused
std::string launchable(const ConvDesc &d) {
    if (!d.sx) {
        for (bool vec4 : {true, false})
            if (!conv_stage(d.cfg, d.K, d.dil, d.padL, d.CK, vec4).fits) return std::string("f32 tile ") + std::to_string(d.cfg) + (vec4 ? " (16-byte DMA)" : " (4-byte DMA)");
        return "";
    }
    const int planes = d.h1 ? 1 : (d.f16 ? 2 : 3);
    int tiles = 0;
    for (int run = 0; run < 4; run++) {
        if (!sx_tile_reads(d.cfg, run, d.s16) || (d.rawin && run != d.cfg)) continue;
        tiles++;
        const SxStage g = sx_stage(sx_tile_n(run), d.K, d.dil, planes, d.s16);
        if (!g.fits || (d.rawin && !g.raw_ok)) return "sx tile " + std::to_string(run);
    }
    if (d.rawin && d.cfg == 0) return "raw input on the 128-row tile";
    return tiles ? "" : "no tile";
}

std::string row(const Format &f, int Cin, int Cout, int K, int x, const std::string &err, const ConvDesc &d) {
    std::string r = std::string(f.name) + " " + std::to_string(Cin) + " " + std::to_string(Cout) + " " + std::to_string(K) + " " + std::to_string(x);
    if (!err.empty()) return r + " R " + err + "\n";
    const std::string v = launchable(d);
    return r + (v.empty() ? " A\n" : " V " + v + "\n");
}

}  // namespace

int main() {
    const std::vector<int> Ks = {1, 2, 3, 5, 7, 11, 13}, Ds = {1, 2, 3, 5, 9, 12, 16, 27, 32}, Cis = {16, 32, 64, 96, 128, 512},
                           Cos = {32, 64, 128, 192, 512};
    const int TK[5] = {16, 8, 4, 3, 7}, TU[5] = {8, 4, 2, 1, 3};  // transposed convs: K - 2 * pad == stride
    const std::vector<Format> fm = formats();
    const std::vector<float> zeros(size_t(512) * 512 * 16, 0.f);  // (the geometry does not depend on the weights)
    struct Job {
        int Cin, Cout, K;  // K < 0: the transposed convs of (Cin, Cout)
    };
    std::vector<Job> jobs;
    for (int Cin : Cis)
        for (int Cout : Cos) {
            for (int K : Ks) jobs.push_back({Cin, Cout, K});
            jobs.push_back({Cin, Cout, -1});
        }
    std::vector<std::string> out(jobs.size());
    std::atomic<size_t> next{0};
    auto work = [&] {
        for (size_t j; (j = next++) < jobs.size();) {
            const Job &jb = jobs[j];
            std::string &o = out[j];
            if (jb.K > 0) {
                for (int dil : Ds)
                    for (const Format &f : fm) {
                        ConvDesc d;
                        std::vector<float> arena;
                        const std::string e = pack_test_conv(zeros.data(), zeros.data(), jb.Cin, jb.Cout, jb.K, dil, dil * (jb.K - 1) / 2, f.hint, &d, &arena, f.o);
                        o += row(f, jb.Cin, jb.Cout, jb.K, dil, e, d);
                    }
                continue;
            }
            for (int t = 0; t < 5; t++)
                for (const Format &f : fm) {
                    if (f.hint == 1 || f.hint == 2) continue;  // (pack_test_convT takes no size class)
                    ConvDesc d;
                    std::vector<float> arena;
                    const std::string e = pack_test_convT(zeros.data(), zeros.data(), jb.Cin, jb.Cout, TK[t], TU[t], &d, &arena, f.hint == 3, f.o);
                    Format tf = f;
                    const std::string name = std::string("T_") + f.name;
                    tf.name = name.c_str();
                    o += row(tf, jb.Cin, jb.Cout, TK[t], TU[t], e, d);
                }
        }
    };
    unsigned nt = std::thread::hardware_concurrency();
    nt = nt < 1 ? 1 : (nt > 16 ? 16 : nt);
    std::vector<std::thread> th;
    for (unsigned i = 0; i < nt; i++) th.emplace_back(work);
    for (auto &t : th) t.join();
    for (const auto &o : out) fputs(o.c_str(), stdout);
    return 0;
}
