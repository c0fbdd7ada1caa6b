// Driver of test_limit_cpu.py: limit.hpp + workspace.hpp under the host compiler, no HIP.  Reads cases from the file named on
// the command line - the test writes them from tests/limit_ref.py, so both sides see the same inputs - and prints one JSON
// object per case:
//   C n_segs / n_segs records "mode ceiling_bits lookahead reserved volume_bits"
//       -> {"check": "<limit_fault's message>"}
//   G ceiling_bits lookahead c / c values "bits"
//       -> {"gain": [the bits of limit_gains' g[0 .. c)], "q": [limit_q of every value]}
// (a float travels as the hexadecimal bits of its value).  Then one line per batch size for the workspace walk of the
// limiter's buffers.
#include <cinttypes>
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include "delivery_walk_check.hpp"
#include "limit.hpp"
#include "workspace.hpp"

using namespace vitsmi;

namespace {

bool read_float(FILE *f, float &v) {
    uint32_t bits;
    if (fscanf(f, "%" SCNx32, &bits) != 1) return false;
    std::memcpy(&v, &bits, 4);
    return true;
}

uint32_t bits_of(float v) {
    uint32_t b;
    std::memcpy(&b, &v, 4);
    return b;
}

}  // namespace

int main(int argc, char **argv) {
    if (argc < 2) return 2;
    FILE *f = fopen(argv[1], "r");
    if (!f) return 2;
    int cases = 0;
    if (fscanf(f, "%d", &cases) != 1) return 2;
    for (int t = 0; t < cases; t++) {
        char kind[4];
        if (fscanf(f, "%3s", kind) != 1) return 3;
        if (kind[0] == 'C') {
            int n_segs;
            if (fscanf(f, "%d", &n_segs) != 1) return 3;
            std::vector<vits_limit> limits(n_segs);
            std::vector<vits_segment> segs(n_segs);
            for (int g = 0; g < n_segs; g++) {
                segs[g] = vits_segment{g, 0, 0, 0, 1.0f};
                if (fscanf(f, "%d", &limits[g].mode) != 1 || !read_float(f, limits[g].ceiling) ||
                    fscanf(f, "%d %d", &limits[g].lookahead, &limits[g].reserved) != 2 || !read_float(f, segs[g].volume))
                    return 3;
            }
            const std::string e = limit_fault(limits.data(), segs.data(), n_segs);
            printf("{\"check\":\"%s\"}\n", e.c_str());
        } else {
            vits_limit l{1, 0.f, 0, 0};
            long long c;
            if (!read_float(f, l.ceiling) || fscanf(f, "%d %lld", &l.lookahead, &c) != 2) return 3;
            std::vector<float> u((size_t)c), g((size_t)c);
            for (auto &v : u)
                if (!read_float(f, v)) return 3;
            const std::string e = limit_fault(&l, nullptr, 1);
            if (!e.empty()) {
                printf("{\"error\":\"%s\"}\n", e.c_str());
                continue;
            }
            limit_gains(u.data(), c, l.ceiling, l.lookahead, g.data());
            printf("{\"gain\":[");
            for (long long j = 0; j < c; j++) printf("%s%u", j ? "," : "", bits_of(g[(size_t)j]));
            printf("],\"q\":[");
            for (long long j = 0; j < c; j++) printf("%s%d", j ? "," : "", limit_q(u[(size_t)j], l.ceiling));
            printf("]}\n");
        }
    }
    fclose(f);
    // the limiter's walk: a record per segment and a float per sample, behind the shape tables - dry against real; the one
    // walk of a delivery call carves the same with the limiter on, and what it carved before with it off
    for (int B : {1, 3, 32, 256}) {
        const int S = 4097;
        const int64_t n_knots = B;
        Carver dry;
        carve_delivery(dry, B, S);
        carve_trim(dry, B);
        carve_level(dry, B, S);
        carve_shape(dry, B, n_knots);
        const size_t shape = dry.used;
        const LimitBufs l0 = carve_limit(dry, B, S);
        char *const base = reinterpret_cast<char *>(uintptr_t(1) << 44);
        Carver real(base, dry.used);
        carve_delivery(real, B, S);
        carve_trim(real, B);
        carve_level(real, B, S);
        const ShapeBufs sb = carve_shape(real, B, n_knots);
        const LimitBufs l = carve_limit(real, B, S);
        Carver one(base, dry.used);
        const DeliveryCallBufs cb = carve_delivery_call(one, B, S, DeliveryNeeds{true, true, true, n_knots, true});
        Carver off(base, dry.used);
        const DeliveryCallBufs cb0 = carve_delivery_call(off, B, S, DeliveryNeeds{true, true, true, n_knots});
        const bool ok = !l0.segs && !l0.gain && real.fits() && real.used == dry.used && sizeof(LimitSeg) == 16 && sizeof(vits_limit) == 16 &&
                        (char *)l.segs >= (char *)sb.knots + sizeof(ShapeKnot) * (size_t)n_knots &&
                        (char *)l.gain >= (char *)l.segs + sizeof(LimitSeg) * (size_t)B && (uintptr_t)l.gain % 16 == 0 &&
                        (char *)l.gain + sizeof(float) * (size_t)B * S <= base + real.used && one.fits() && one.used == real.used &&
                        cb.limit.segs == l.segs && cb.limit.gain == l.gain && cb.shape.knots == sb.knots && off.used == shape &&
                        !cb0.limit.segs && !cb0.limit.gain && cb0.shape.knots == sb.knots &&
                        delivery_call_walk_agrees(B, S);  // (and without the limiter the one walk is what it was)
        printf("{\"walk\":%d,\"ok\":%d,\"shape\":%zu,\"with_limit\":%zu,\"record\":%zu}\n", B, (int)ok, shape, dry.used, sizeof(LimitSeg));
    }
    return 0;
}
