// Driver of test_stream_pack_cpu.py: workspace.hpp + slab.hpp under the host compiler, no HIP.  Walks the encoded stream's
// workspace (carve_stream, the one walk of a streamed run) - alone (a native run carves it from the staging slab's base) and
// behind carve_resample's buffers (a run at an output rate) - over a grid of request sizes: once dry, once over a fake base (never
// dereferenced), once with one byte too little; and places a chunk of every encoding and of several lengths up to n_max to see
// that its bytes start inside the buffer, 16-byte aligned, and end exactly at the running peaks.  One line per (B, n_max, K):
//   <B> <n_max> <K> A <stream pack bytes> <resample + stream pack bytes>     every check held
//   <B> <n_max> <K> V <what>                                                 a check failed
// The extents below are what the kernel and the copy need of each buffer, written here independently of the walk.
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
        if ((p - kBase) % 16) return std::string(plan) + ": " + ex[i].name + " is not 16-byte aligned";
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

size_t round16(size_t v) { return (v + 15) / 16 * 16; }

// the largest chunk (F32) in whole 16-byte cells per row; a float per row for the peaks, in whole cells; two floats per row
void stream_extents(std::vector<Ext> &e, const StreamPackBufs &s, int B, size_t n_max) {
    e.push_back({"chunk", s.buf, (size_t)B * round16(4 * n_max)});
    e.push_back({"peak_run", s.peak_run, round16((size_t)B * 4)});
    e.push_back({"fmt", s.fmt, (size_t)B * 2 * 4});
}

std::vector<Ext> alone(Carver &cv, int B, size_t n_max, std::string *placed) {
    std::vector<Ext> e;
    const StreamPackBufs s = carve_stream(cv, B, (int64_t)n_max, (int64_t)n_max, /*K=*/0, /*enc=*/true, /*shaped=*/false, 0, 0).sp;
    stream_extents(e, s, B, n_max);
    if (cv.base && placed) {
        // a chunk of n samples at w bytes: [B][pitch] bytes that end at the peaks
        const size_t ns[] = {1, 2, 7, 16, n_max / 2 + 1, n_max};
        for (int w : {1, 2, 4})
            for (size_t n : ns) {
                if (n > n_max) continue;
                const size_t pitch = round16(w * n);
                if (StreamPackBufs::pitch(w, (int64_t)n) != pitch) *placed = "pitch(" + std::to_string(w) + ", " + std::to_string(n) + ")";
                const unsigned char *d = s.at(B, pitch);
                if (d < s.buf || (d - s.buf) % 16) *placed = "a chunk starts outside the buffer or off a cell";
                if ((const void *)(d + (size_t)B * pitch) != (const void *)s.peak_run) *placed = "a chunk does not end at the peaks";
            }
        if ((const char *)s.fmt != (const char *)s.peak_run + round16((size_t)B * 4)) *placed = "the format table is not behind the peaks";
    }
    return e;
}

std::vector<Ext> resampled(Carver &cv, int B, size_t S, int K, size_t n_max) {
    const StreamBufs sb = carve_stream(cv, B, (int64_t)S, (int64_t)n_max, K, /*enc=*/true, /*shaped=*/false, 0, 0);
    const ResampleBufs &r = sb.rs;
    std::vector<Ext> e = {{"out", r.out, (size_t)B * S * 4}, {"n_in", r.n_in, (size_t)B * 4}, {"n_out", r.n_out, (size_t)B * 4},
                          {"carry0", r.carry[0], (size_t)B * K * 4}, {"carry1", r.carry[1], (size_t)B * K * 4},
                          {"pcm", r.pcm.pcm, (size_t)B * S * 2}, {"pcm peak", r.pcm.peak, (size_t)B * 4},
                          {"packed", r.dlv.packed, round16((size_t)B * S * 4)}, {"segs", r.dlv.segs, (size_t)B * 32},
                          {"peak", r.dlv.peak, (size_t)B * 2 * 4}};
    const StreamPackBufs &s = sb.sp;
    stream_extents(e, s, B, n_max);
    if (cv.base && (const char *)s.buf < (const char *)r.dlv.peak) e.push_back({"stream pack (behind the resampler's buffers)", nullptr, 0});
    return e;
}

}  // namespace

int main() {
    const int Bs[] = {1, 2, 3, 7, 32, 256}, Ns[] = {1, 3, 96, 4097, 16384, 2000000}, Ks[] = {38, 104};
    for (int B : Bs)
        for (int N : Ns)
            for (int K : Ks) {
                printf("%d %d %d ", B, N, K);
                size_t sp = 0, rs = 0;
                std::string placed;
                std::string v = check("stream pack", [&](Carver &cv) { return alone(cv, B, (size_t)N, &placed); }, &sp);
                if (v.empty()) v = placed;
                // (at an output rate a chunk never holds more than the whole row: S >= n_max)
                if (v.empty()) v = check("resampled", [&](Carver &cv) { return resampled(cv, B, (size_t)N + 5, K, (size_t)N); }, &rs);
                if (v.empty()) printf("A %zu %zu\n", sp, rs);
                else printf("V %s\n", v.c_str());
            }
    return 0;
}
