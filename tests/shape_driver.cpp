// Driver of test_shape_cpu.py: shape.hpp + workspace.hpp under the host compiler, no HIP.  Reads cases from the file named
// on the command line - the test writes them from tests/shape_ref.py, so both sides see the same inputs - and prints one JSON
// object per case:
//   C n_segs n_points_stated n_given / n_segs records "fade_in fade_out curve n_points first_point" / n_given points "pos bits"
//       -> {"check": "<shape_fault's message>"}
//   G fade_in fade_out curve n_given a c / n_given points
//       -> {"gain": [the bits of shape_gain at row samples a .. a + c - 1, through shape_table and shape_slopes],
//           "knots": 1 when shape_gain_knots - the form the kernel runs, over shape_knots' records - gives the same bits}
// (a gain travels as the hexadecimal bits of its float).  Then one line for the workspace walk of the shape tables.
#include <cinttypes>
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include "delivery_walk_check.hpp"
#include "workspace.hpp"

using namespace vitsmi;

namespace {

bool read_points(FILE *f, int n, std::vector<vits_env_point> &pts) {
    pts.resize(n);
    for (int k = 0; k < n; k++) {
        uint32_t bits;
        if (fscanf(f, "%d %" SCNx32, &pts[k].pos, &bits) != 2) return false;
        std::memcpy(&pts[k].gain, &bits, 4);
    }
    return true;
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
        std::vector<vits_env_point> pts;
        if (kind[0] == 'C') {
            int n_segs, n_given;
            long long stated;
            if (fscanf(f, "%d %lld %d", &n_segs, &stated, &n_given) != 3) return 3;
            std::vector<vits_shape> shapes(n_segs);
            for (auto &s : shapes) {
                long long first;
                if (fscanf(f, "%d %d %d %d %lld", &s.fade_in, &s.fade_out, &s.curve, &s.n_points, &first) != 5) return 3;
                s.first_point = first;
            }
            if (!read_points(f, n_given, pts)) return 3;
            const std::string e = shape_fault(shapes.data(), n_segs, pts.data(), stated);
            printf("{\"check\":\"%s\"}\n", e.c_str());
        } else {
            vits_shape s{};
            int n_given;
            long long a, c;
            if (fscanf(f, "%d %d %d %d %lld %lld", &s.fade_in, &s.fade_out, &s.curve, &n_given, &a, &c) != 6) return 3;
            if (!read_points(f, n_given, pts)) return 3;
            s.n_points = n_given;
            s.first_point = 0;
            const std::string e = shape_fault(&s, 1, pts.data(), n_given);
            if (!e.empty()) {
                printf("{\"error\":\"%s\"}\n", e.c_str());
                continue;
            }
            std::vector<ShapeSeg> table;
            std::vector<float> slopes;
            const int64_t a64 = a, c64 = c;
            shape_table(&s, std::vector<int>{0}, &a64, &c64, table);
            shape_slopes(pts.data(), n_given, slopes);
            std::vector<ShapeSeg> ktable(table);
            std::vector<ShapeKnot> knots;
            shape_knots(ktable, pts.data(), knots);
            bool same = knots.size() == (size_t)n_given + 1 && knots.back().next == INT_MAX && knots.back().slope == 0.f;
            printf("{\"gain\":[");
            for (long long j = 0; j < c; j++) {
                const float m = shape_gain(table[0], pts.data(), slopes.data(), (int32_t)(a + j));
                const float mk = shape_gain_knots(ktable[0], knots.data(), (int32_t)(a + j));
                uint32_t bits, kbits;
                std::memcpy(&bits, &m, 4);
                std::memcpy(&kbits, &mk, 4);
                same = same && bits == kbits;
                printf("%s%u", j ? "," : "", bits);
            }
            printf("],\"knots\":%d}\n", (int)same);
        }
    }
    fclose(f);
    // the shape tables' walk: a record per segment and sixteen bytes per knot, behind the level buffers
    for (int B : {1, 3, 32, 256}) {
        const int64_t n_points = 1000 + B;  // (knots)
        Carver dry;
        carve_delivery(dry, B, 4097);
        carve_trim(dry, B);
        carve_level(dry, B, 4097);
        const size_t level = dry.used;
        const ShapeBufs s0 = carve_shape(dry, B, n_points);
        char *const base = reinterpret_cast<char *>(uintptr_t(1) << 44);
        Carver real(base, dry.used);
        carve_delivery(real, B, 4097);
        carve_trim(real, B);
        const LevelBufs l = carve_level(real, B, 4097);
        const ShapeBufs s = carve_shape(real, B, n_points);
        const bool ok = !s0.segs && !s0.knots && real.fits() && real.used == dry.used && sizeof(ShapeKnot) == 16 &&
                        (char *)s.segs >= (char *)l.result + 4 * (l.n_peaks + l.n_subs) &&
                        (char *)s.knots >= (char *)s.segs + sizeof(ShapeSeg) * (size_t)B && (uintptr_t)s.knots % 16 == 0 &&
                        (char *)s.knots + 16 * (size_t)n_points <= base + real.used &&
                        delivery_call_walk_agrees(B, 4097);  // (and the one walk of a delivery call carves the same)
        printf("{\"walk\":%d,\"ok\":%d,\"level\":%zu,\"with_shape\":%zu,\"points\":%lld,\"record\":%zu}\n", B, (int)ok, level, dry.used,
               (long long)n_points, sizeof(ShapeSeg));
    }
    return 0;
}
