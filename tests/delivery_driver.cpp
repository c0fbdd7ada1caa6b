// Driver of test_delivery_cpu.py: workspace.hpp + delivery.hpp + slab.hpp under the host compiler, no HIP.  Walks the
// delivery workspace - on its own (a native run carves it from the staging slab's base) and inside the resampled result's
// walk (behind the PCM buffers) - over a grid of request sizes: once dry, once over a fake base (never dereferenced), once
// with one byte too little; and lays out the largest plan a request admits (every row, F32) to see that it fits.  One line
// per (B, S, K):
//   <B> <S> <K> A <delivery bytes> <resample walk bytes>     every check held
//   <B> <S> <K> V <what>                                     a check failed
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

// the packed audio in whole 16-byte cells (F32, every sample of every row), a 32-byte record per row, a peak per row and stream
void delivery_extents(std::vector<Ext> &e, const DeliveryBufs &d, int B, size_t S) {
    e.push_back({"packed", d.packed, ((size_t)B * S * 4 + 15) / 16 * 16});
    e.push_back({"segs", d.segs, (size_t)B * 32});
    e.push_back({"peak", d.peak, (size_t)B * 2 * 4});
}

std::vector<Ext> delivery(Carver &cv, int B, size_t S) {
    std::vector<Ext> e;
    delivery_extents(e, carve_delivery(cv, B, (int)S), B, S);
    return e;
}

std::vector<Ext> resampled(Carver &cv, int B, size_t S, int K) {
    const ResampleBufs r = carve_resample(cv, B, (int)S, K);
    std::vector<Ext> e = {{"out", r.out, (size_t)B * S * 4}, {"n_in", r.n_in, (size_t)B * 4}, {"n_out", r.n_out, (size_t)B * 4},
                          {"carry0", r.carry[0], (size_t)B * K * 4}, {"carry1", r.carry[1], (size_t)B * K * 4},
                          {"pcm", r.pcm.pcm, (size_t)B * S * 2}, {"pcm peak", r.pcm.peak, (size_t)B * 4}};
    delivery_extents(e, r.dlv, B, S);
    if (cv.base && (const char *)r.dlv.packed < (const char *)r.pcm.peak) e.push_back({"delivery (behind the PCM buffers)", nullptr, 0});
    return e;
}

// the largest plan of a request: every row a segment of S samples, F32, leads in between - what the device side must hold
std::string largest_plan(int B, int S) {
    std::vector<int64_t> counts(B, S);
    std::vector<vits_segment> segs(B);
    for (int b = 0; b < B; b++) segs[b] = vits_segment{B - 1 - b, b % ((B + 1) / 2), b % 3, b % 3, 1.0f};
    DeliveryPlan p;
    const std::string err = delivery_plan(counts.data(), B, S, segs.data(), B, (B + 1) / 2, VITS_ENC_F32, p);
    if (!err.empty()) return "plan refused: " + err;
    if ((size_t)(p.packed_elems * 4 + 15) / 16 * 16 > (size_t)B * S * 4 + 16) return "the packed audio exceeds its buffer";
    if (p.segs.size() > (size_t)B) return "more segment records than rows";
    int64_t copied = 0;
    for (const DeliveryCopy &c : p.copies) {
        if (c.packed_off < 0 || c.packed_off + c.bytes > p.packed_elems * 4 || c.dst_off + c.bytes > p.total_bytes) return "a copy leaves its buffers";
        copied += c.bytes;
    }
    if (copied != p.packed_elems * 4) return "the copies do not cover the packed audio";
    for (const DeliverySeg &s : p.segs)
        if (s.peak >= 2 * B || s.src + s.n > (int64_t)B * S) return "a segment record points outside the request";
    return "";
}

}  // namespace

int main() {
    const int Bs[] = {1, 2, 3, 8, 32, 256}, Ss[] = {1, 3, 96, 4097, 40000, 2000000}, Ks[] = {38, 104};
    for (int B : Bs)
        for (int S : Ss)
            for (int K : Ks) {
                printf("%d %d %d ", B, S, K);
                size_t dlv = 0, rs = 0;
                std::string v = check("delivery", [&](Carver &cv) { return delivery(cv, B, (size_t)S); }, &dlv);
                if (v.empty()) v = check("resampled", [&](Carver &cv) { return resampled(cv, B, (size_t)S, K); }, &rs);
                if (v.empty() && S <= 40000) v = largest_plan(B, S);
                if (v.empty()) printf("A %zu %zu\n", dlv, rs);
                else printf("V %s\n", v.c_str());
            }
    return 0;
}
