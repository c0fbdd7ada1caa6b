// Driver of test_trim_cpu.py: delivery.hpp + workspace.hpp under the host compiler, no HIP.  Draws seeded random plans of a
// trimmed delivery - rows with their active bounds at either end, in the middle, absent, rows without samples; margins that
// overlap or run off either end; tails with and without leads; every third plan without trims at all - runs trim_range and
// the plan over them and prints one JSON object per plan: the inputs, so that the test can state them to its reference,
// and everything the plan answered.  Then one line for the workspace walk of the trim slots.
#include <cstdio>
#include <string>
#include <vector>

#include "delivery_walk_check.hpp"
#include "workspace.hpp"

using namespace vitsmi;

namespace {

uint64_t g_state = 0x9E3779B97F4A7C15ull;
uint32_t rnd() {  // splitmix64's high half
    uint64_t z = (g_state += 0x9E3779B97F4A7C15ull);
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return (uint32_t)((z ^ (z >> 31)) >> 32);
}
int pick(std::initializer_list<int> v) { return v.begin()[rnd() % v.size()]; }

template <class T, class F>
void list(const char *name, const std::vector<T> &v, F &&one, bool last = false) {
    printf("\"%s\":[", name);
    for (size_t i = 0; i < v.size(); i++) {
        if (i) printf(",");
        one(v[i]);
    }
    printf("]%s", last ? "" : ",");
}

}  // namespace

int main() {
    const int64_t S = 1000;  // the rows' pitch
    for (int plan = 0; plan < 400; plan++) {
        const int B = 1 + rnd() % 7, J = 1 + rnd() % B, enc = rnd() % 4;
        const bool with_trims = plan % 3 != 2;
        std::vector<int64_t> counts(B), f(B), l(B), first(B), kept(B);
        for (int b = 0; b < B; b++) {
            counts[b] = pick({0, 1, 2, 7, 40, 40, 64});
            const int n = (int)counts[b];
            const int kind = n == 0 ? 0 : rnd() % 6;
            switch (kind) {
                case 0: f[b] = INT_MAX, l[b] = -1; break;                       // none active
                case 1: f[b] = 0, l[b] = n - 1; break;                          // both ends
                case 2: f[b] = 0, l[b] = rnd() % n; break;                      // the front end
                case 3: f[b] = rnd() % n, l[b] = n - 1; break;                  // the back end
                case 4: f[b] = l[b] = rnd() % n; break;                         // exactly one
                default: f[b] = rnd() % n, l[b] = f[b] + rnd() % (n - f[b]);    // anywhere
            }
        }
        // a random subset of the rows, in a random order
        std::vector<int> rows(B);
        for (int b = 0; b < B; b++) rows[b] = b;
        for (int b = B - 1; b > 0; b--) std::swap(rows[b], rows[rnd() % (b + 1)]);
        const int G = rnd() % (B + 1);
        std::vector<vits_segment> segs(G);
        std::vector<vits_trim> trims(G);
        for (int g = 0; g < G; g++) {
            segs[g] = vits_segment{rows[g], (int32_t)(rnd() % J), pick({0, 0, 1, 4}), (int32_t)(rnd() % 3), 1.0f};
            trims[g] = vits_trim{(int32_t)(rnd() % 3), 0.25f, pick({0, 1, 3, 100}), pick({0, 1, 3, 100}), pick({0, 0, 2, 5})};
        }
        for (int b = 0; b < B; b++) first[b] = 0, kept[b] = counts[b];
        for (int g = 0; g < G && with_trims; g++) {
            const int r = segs[g].row;
            trim_range(counts[r], f[r], l[r], trims[g], first[r], kept[r]);
        }
        DeliveryPlan p;
        const std::string err = with_trims ? delivery_plan(kept.data(), B, S, segs.data(), G, J, enc, p, trims.data(), first.data())
                                           : delivery_plan(counts.data(), B, S, segs.data(), G, J, enc, p);
        printf("{\"B\":%d,\"J\":%d,\"enc\":%d,\"with_trims\":%d,\"err\":\"%s\",", B, J, enc, (int)with_trims, err.c_str());
        list("counts", counts, [](int64_t v) { printf("%lld", (long long)v); });
        list("f", f, [](int64_t v) { printf("%lld", (long long)v); });
        list("l", l, [](int64_t v) { printf("%lld", (long long)v); });
        list("first", first, [](int64_t v) { printf("%lld", (long long)v); });
        list("kept", kept, [](int64_t v) { printf("%lld", (long long)v); });
        list("segs", segs, [](const vits_segment &s) { printf("[%d,%d,%lld,%d]", s.row, s.stream, (long long)s.lead_samples, s.normalize); });
        list("trims", trims, [](const vits_trim &t) { printf("[%d,%d,%d,%lld]", t.mode, t.keep_lead, t.keep_tail, (long long)t.tail_samples); });
        list("samples", p.stream_samples, [](int64_t v) { printf("%lld", (long long)v); });
        list("offsets", p.stream_offsets, [](int64_t v) { printf("%lld", (long long)v); });
        list("order", p.order, [](int v) { printf("%d", v); });
        list("table", p.segs, [](const DeliverySeg &d) { printf("[%lld,%lld,%d,%d]", (long long)d.start, (long long)d.src, d.n, d.peak); });
        list("copies", p.copies, [](const DeliveryCopy &c) { printf("[%lld,%lld,%lld]", (long long)c.packed_off, (long long)c.dst_off, (long long)c.bytes); });
        list("fills", p.fills, [](const DeliveryFill &c) { printf("[%lld,%lld]", (long long)c.dst_off, (long long)c.elems); });
        printf("\"width\":%d,\"packed\":%lld,\"total\":%lld,\"max_n\":%d}\n", p.width, (long long)p.packed_elems, (long long)p.total_bytes, p.max_n);
    }
    // the trim slots' walk: two int32 per segment and a peak per segment, behind the delivery's buffers
    for (int B : {1, 3, 32, 256}) {
        Carver dry;
        carve_delivery(dry, B, 4097);
        const size_t dlv = dry.used;
        const TrimBufs t0 = carve_trim(dry, B);
        char *const base = reinterpret_cast<char *>(uintptr_t(1) << 44);
        Carver real(base, dry.used);
        const DeliveryBufs d = carve_delivery(real, B, 4097);
        const TrimBufs t = carve_trim(real, B);
        const bool ok = !t0.bounds && !t0.peak_all && real.fits() && real.used == dry.used &&
                        (char *)t.bounds >= (char *)d.peak + 8 * (size_t)B && (char *)t.peak_all >= (char *)t.bounds + 8 * (size_t)B &&
                        (char *)t.peak_all + 4 * (size_t)B <= base + real.used &&
                        delivery_call_walk_agrees(B, 4097);  // (and the one walk of a delivery call carves the same)
        printf("{\"walk\":%d,\"ok\":%d,\"delivery\":%zu,\"with_trim\":%zu}\n", B, (int)ok, dlv, dry.used);
    }
    return 0;
}
