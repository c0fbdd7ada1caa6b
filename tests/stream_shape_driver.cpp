// Driver of test_stream_shape_cpu.py: workspace.hpp + stream_shape.hpp under the host compiler, no HIP.  Walks the shaped
// stream's workspace - carve_stream, the one walk of a streamed run: the chunk buffer for n_max + L samples, the shaped
// stream's tables behind it; alone (a native run) and behind carve_resample's buffers (a run at an output rate) - over a grid
// of request sizes: once dry, once over a fake base (never dereferenced), once with one byte too little.  Then the plan's host
// code on real memory: the rows' records and knots of a shaping (stream_shape_table), and the timeline over pieces of several
// sizes.  Last the size arithmetic of a streamed run (stream_n_max, stream_ring_bytes) along the pipeline's own piece
// schedule: chunks of frames, through the resampler's completion rule, through the look-ahead.  Lines:
//   walk <B> <n_max> <L> <knots> A <alone bytes> <behind the resampler bytes>     every check held
//   walk <B> <n_max> <L> <knots> V <what>                                         a check failed
//   table <rows> <knots> <first knot of every row ...>
//   emit <L> <piece> <total> <first n ...>                                        the delivered range of every piece
//   sched <hop> <chunk> <F> <out rate, 0: none> <L> <total> <n_max> <ring bytes: fp32 (L = 0; else 0), 1, 2, 4 bytes wide>
//         <first n ...>                                 B = kSchedB rows at 22050 Hz: what every chunk delivers, n = 0 included
// The extents below are what the kernels need of each buffer, written here independently of the walk.
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

// the chunk of n_max + L samples (F32) in whole cells per row, the peaks, the format table; a 32-byte record per row, a
// 16-byte knot each, two carries of 2 L floats per row
void shaped_extents(std::vector<Ext> &e, const Carver &cv, const StreamBufs &sb, int B, size_t n_max, int L, size_t knots) {
    const StreamPackBufs &s = sb.sp;
    const StreamShapeBufs &ss = sb.ss;
    e.push_back({"chunk", s.buf, (size_t)B * round16(4 * (n_max + L))});
    e.push_back({"peak_run", s.peak_run, round16((size_t)B * 4)});
    e.push_back({"fmt", s.fmt, (size_t)B * 2 * 4});
    e.push_back({"rows", ss.rows, (size_t)B * 32});
    e.push_back({"knots", ss.knots, knots * 16});
    if (L > 0) {  // (without a look-ahead the carries have no bytes: nothing reads them)
        e.push_back({"carry0", ss.carry[0], (size_t)B * 2 * L * 4});
        e.push_back({"carry1", ss.carry[1], (size_t)B * 2 * L * 4});
    }
    if (cv.base && (const char *)ss.rows < (const char *)s.fmt) e.push_back({"stream shape (behind the stream pack's buffers)", nullptr, 0});
}

std::vector<Ext> alone(Carver &cv, int B, size_t n_max, int L, size_t knots) {
    std::vector<Ext> e;
    const StreamBufs sb = carve_stream(cv, B, (int64_t)(n_max + L), (int64_t)(n_max + L), /*K=*/0, /*enc=*/true, /*shaped=*/true, L, (int64_t)knots);
    shaped_extents(e, cv, sb, B, n_max, L, knots);
    return e;
}

std::vector<Ext> resampled(Carver &cv, int B, size_t S, int K, size_t n_max, int L, size_t knots) {
    const StreamBufs sb = carve_stream(cv, B, (int64_t)S, (int64_t)(n_max + L), K, /*enc=*/true, /*shaped=*/true, L, (int64_t)knots);
    const ResampleBufs &r = sb.rs;
    std::vector<Ext> e = {{"out", r.out, (size_t)B * S * 4}, {"n_in", r.n_in, (size_t)B * 4}, {"n_out", r.n_out, (size_t)B * 4},
                          {"carry0 (resampler)", r.carry[0], (size_t)B * K * 4}, {"carry1 (resampler)", r.carry[1], (size_t)B * K * 4},
                          {"pcm", r.pcm.pcm, (size_t)B * S * 2}, {"pcm peak", r.pcm.peak, (size_t)B * 4},
                          {"packed", r.dlv.packed, round16((size_t)B * S * 4)}, {"segs", r.dlv.segs, (size_t)B * 32},
                          {"peak", r.dlv.peak, (size_t)B * 2 * 4}};
    shaped_extents(e, cv, sb, B, n_max, L, knots);
    return e;
}

constexpr int kSchedB = 3;

// one streamed run of F frames in chunks of `chunk`, as render_chunks walks it: every chunk's input samples through
// resample_emit_end (an output rate) and stream_emit_range (the look-ahead; an empty completion is not handed on)
void schedule(int hop, int chunk, int F, int fo, int L) {
    ResamplePlan rp;
    if (fo && !resample_plan(22050, fo, rp).empty()) {
        printf("sched %d %d %d %d %d bad plan\n", hop, chunk, F, fo, L);
        return;
    }
    const int64_t total = rp.on() ? rp.count((int64_t)F * hop) : (int64_t)F * hop, n_max = stream_n_max(rp, chunk, F, hop, L, total);
    printf("sched %d %d %d %d %d %lld %lld %zu %zu %zu %zu", hop, chunk, F, fo, L, (long long)total, (long long)n_max,
           L ? (size_t)0 : stream_ring_bytes(kSchedB, n_max, 0), stream_ring_bytes(kSchedB, n_max, 1), stream_ring_bytes(kSchedB, n_max, 2),
           stream_ring_bytes(kSchedB, n_max, 4));
    int64_t emitted = 0;
    for (int f0 = 0; f0 < F; f0 += chunk) {
        const int f1 = f0 + chunk < F ? f0 + chunk : F;
        int64_t first = (int64_t)f0 * hop, n = (int64_t)(f1 - f0) * hop;
        if (rp.on()) {
            const int64_t hi = resample_emit_end(rp, first + n, f1 == F, total);
            first = emitted;
            n = hi > emitted ? hi - emitted : 0;
            emitted += n;
        }
        if (n > 0) stream_emit_range(first, n, first + n >= total, total, L, first, n);
        printf(" %lld %lld", (long long)first, (long long)n);
    }
    printf("\n");
}

}  // namespace

int main() {
    static_assert(sizeof(StreamShapeRow) == 32 && sizeof(ShapeKnot) == 16 && sizeof(vits_stream_shaping) == 56, "record sizes");
    const int Bs[] = {1, 3, 32, 256}, Ns[] = {1, 96, 4097, 16384, 2000000}, Ls[] = {0, 1, 110, 1024};
    for (int B : Bs)
        for (int N : Ns)
            for (int L : Ls) {
                const size_t knots = (size_t)B * (L ? 81 : 1);  // (two breakpoints per token of 40, and one more; or none)
                printf("walk %d %d %d %zu ", B, N, L, knots);
                size_t sp = 0, rs = 0;
                std::string v = check("shaped stream", [&](Carver &cv) { return alone(cv, B, (size_t)N, L, knots); }, &sp);
                if (v.empty()) v = check("resampled", [&](Carver &cv) { return resampled(cv, B, (size_t)N + L + 5, 38, (size_t)N, L, knots); }, &rs);
                if (v.empty()) printf("A %zu %zu\n", sp, rs);
                else printf("V %s\n", v.c_str());
            }
    // the plan on real memory: three rows - none, fades, points - and their knots
    {
        const vits_env_point pts[] = {{0, 1.0f}, {10, 0.5f}, {11, 2.0f}, {400, 0.0f}};
        const vits_shape shapes[] = {{0, 0, 0, 0, 0}, {5, 7, 1, 0, 0}, {0, 3, 0, 4, 0}};
        const float ceil[] = {0.5f, 0.f, 1.0f};
        vits_stream_shaping s{};
        s.shapes = shapes;
        s.points = pts;
        s.n_points = 4;
        s.ceiling = ceil;
        s.lookahead = 16;
        std::vector<StreamShapeRow> rows;
        std::vector<ShapeKnot> knots;
        const std::string e = stream_shape_fault(&s, nullptr, 3);
        stream_shape_table(&s, 3, rows, knots);
        printf("table %zu %zu", rows.size(), knots.size());
        for (const auto &r : rows) printf(" %d", r.first);
        printf(" %s\n", e.empty() && (int64_t)knots.size() == stream_knot_count(&s, 3) && rows[1].ceiling == 0.f && rows[2].ceiling == 1.0f ? "ok" : "bad");
        stream_shape_table(nullptr, 2, rows, knots);
        printf("table %zu %zu %d %d ok\n", rows.size(), knots.size(), rows[0].first, rows[1].first);
    }
    for (int L : {0, 1, 7, 255, 1024})
        for (int piece : {1, 7, 255, 256, 1024, 1025, 5000})
            for (int total : {1, 1000, 5000}) {
                printf("emit %d %d %d", L, piece, total);
                for (int64_t f = 0; f < total; f += piece) {
                    int64_t ef, en;
                    const int64_t n = total - f > piece ? piece : total - f;
                    stream_emit_range(f, n, f + n >= total, total, L, ef, en);
                    printf(" %lld %lld", (long long)ef, (long long)en);
                }
                printf("\n");
            }
    for (int hop : {1, 64, 256})
        for (int chunk : {1, 2, 7, 64})
            for (int F : {1, 5, 64, 65})
                for (int fo : {0, 8000, 16000, 44100, 48000})
                    for (int L : {0, 1, 64, 1024}) schedule(hop, chunk, F, fo, L);
    return 0;
}
