// Driver of test_loudness_cpu.py: loudness.hpp + workspace.hpp + slab.hpp under the host compiler, no HIP.  Walks the levelled
// delivery's buffers dry, over a slab of exactly that size and over one a byte short (and holds the one walk of a delivery
// call against the hand-stated sequence: delivery_walk_check.hpp), and checks the chunk-to-chunk
// transition of the filter's state against the recurrence itself.  One JSON object per line.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "delivery_walk_check.hpp"
#include "workspace.hpp"

using namespace vitsmi;

int main() {
    const int shapes[][2] = {{1, 1}, {1, 799}, {3, 1025}, {32, 215040}, {7, 100000}};
    for (const auto &sh : shapes) {
        const int B = sh[0], S = sh[1];
        auto walk = [&](Carver &cv) {
            carve_delivery(cv, B, S);
            carve_trim(cv, B);
            return carve_level(cv, B, S);
        };
        const size_t all = carved_bytes(walk);
        const size_t dlv = carved_bytes([&](Carver &cv) {
            carve_delivery(cv, B, S);
            carve_trim(cv, B);
        });
        std::vector<char> slab(all + 256);
        char *base = reinterpret_cast<char *>((reinterpret_cast<size_t>(slab.data()) + 255) & ~size_t(255));
        Carver real(base, all), tight(base, all - 1);
        const LevelBufs lb = walk(real);
        walk(tight);
        // every buffer inside the slab, the last one ending at its end
        const char *end = reinterpret_cast<const char *>(lb.result + lb.n_peaks + lb.n_subs);
        const bool inside = reinterpret_cast<const char *>(lb.segs) >= base && end == base + all &&
                            reinterpret_cast<const char *>(lb.e()) == reinterpret_cast<const char *>(lb.result) + 4 * lb.n_peaks;
        printf("{\"walk\": 1, \"B\": %d, \"S\": %d, \"Lc\": %d, \"delivery\": %zu, \"level\": %zu, \"fits\": %d, \"short_fits\": %d, "
               "\"chunks\": %zu, \"subs\": %zu, \"peaks\": %zu}\n",
               B, S, kLoudChunk, dlv, all - dlv, (int)(real.fits() && inside && delivery_call_walk_agrees(B, S)), (int)tight.fits(),
               lb.n_chunks, lb.n_subs, lb.n_peaks);
    }
    // the transition: kLoudChunk samples from a state z0 = (the same samples from rest) + M z0
    double c[10], m[16];
    loudness_filter(22050, c);
    loudness_transition(c, kLoudChunk, m);
    double z0[4] = {0.3, -0.2, 0.7, 0.1}, za[4], zb[4] = {0, 0, 0, 0};
    for (int i = 0; i < 4; i++) za[i] = z0[i];
    unsigned r = 12345u;
    for (int i = 0; i < kLoudChunk; i++) {
        r = r * 1664525u + 1013904223u;
        const double x = (double)(r >> 8) / (1 << 24) - 0.5;
        loudness_step(c, x, za);
        loudness_step(c, x, zb);
    }
    double err = 0;
    for (int i = 0; i < 4; i++) {
        double v = zb[i];
        for (int j = 0; j < 4; j++) v += m[4 * i + j] * z0[j];
        err = std::fmax(err, std::fabs(v - za[i]));
    }
    printf("{\"transition\": 1, \"err\": %.3g, \"hop\": %d, \"parts\": %d}\n", err, loudness_coef(22050).hop, kLoudParts);
    return 0;
}
