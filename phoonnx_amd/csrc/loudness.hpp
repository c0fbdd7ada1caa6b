// loudness.hpp — the host side of a levelled delivery (include/vitsmi.h, "levelled delivery"): the K-weighting filter of a
// rate, the chunk-to-chunk transition of its state, the gates of BS.1770-4 over sub-block energies, and the gain.  Host-side
// C++17 in double, no HIP types: pure functions of their arguments, answered without a handle or a device.  The kernels that
// produce the energies: loudness.hip.hpp.
#pragma once
#include <cmath>
#include <cstdint>
#include <limits>
#include <vector>

#include "delivery.hpp"

namespace vitsmi {

// Lc: the samples of a chunk of the chunk-parallel filter (loudness.hip.hpp), counted from the kept range's first sample
constexpr int kLoudChunk = 1024;
// the shortest sub-block: hop of the smallest admitted rate
constexpr int kLoudMinHop = (kLevelMinRate + 5) / 10;
// the sub-blocks one chunk can touch: its first one, the whole ones inside, its last one
constexpr int kLoudParts = (kLoudChunk - 1) / kLoudMinHop + 2;

// one levelled segment as the kernels read it (32 bytes)
struct LoudSeg {
    int64_t src;     // element offset of the kept range's first sample in the waveform
    int64_t chunk0;  // the segment's first slot in fin / init / part (part: times kLoudParts)
    int64_t sub0;    // the segment's first slot in e
    int32_t n;       // n_sub * hop: the samples that count
    int32_t pad;
};

// the four state values of the two biquads, as the kernels keep them per chunk
struct alignas(16) LoudState {
    float x, y, z, w;
};

inline int loudness_hop(int sample_rate) { return (sample_rate + 5) / 10; }

// coef: shelf {b0, b1, b2, a1, a2}, high-pass {b0, b1, b2, a1, a2} (a0 = 1): the analogue prototypes of BS.1770 through the
// bilinear transform
inline void loudness_filter(int sample_rate, double coef[10]) {
    const double pi = 3.14159265358979323846;
    {
        const double f0 = 1681.974450955533, G = 3.999843853973347, Q = 0.7071752369554196;
        const double K = std::tan(pi * f0 / sample_rate), Vh = std::pow(10.0, G / 20.0), Vb = std::pow(Vh, 0.4996667741545416);
        const double a0 = 1.0 + K / Q + K * K;
        coef[0] = (Vh + Vb * K / Q + K * K) / a0;
        coef[1] = 2.0 * (K * K - Vh) / a0;
        coef[2] = (Vh - Vb * K / Q + K * K) / a0;
        coef[3] = 2.0 * (K * K - 1.0) / a0;
        coef[4] = (1.0 - K / Q + K * K) / a0;
    }
    {
        const double f0 = 38.13547087602444, Q = 0.5003270373238773;
        const double K = std::tan(pi * f0 / sample_rate), a0 = 1.0 + K / Q + K * K;
        coef[5] = 1.0;
        coef[6] = -2.0;
        coef[7] = 1.0;
        coef[8] = 2.0 * (K * K - 1.0) / a0;
        coef[9] = (1.0 - K / Q + K * K) / a0;
    }
}

// one sample through the two biquads (transposed direct form II; z: the four state values) - the kernels' step in double
inline double loudness_step(const double c[10], double x, double z[4]) {
    const double y1 = c[0] * x + z[0];
    z[0] = c[1] * x - c[3] * y1 + z[1];
    z[1] = c[2] * x - c[4] * y1;
    const double y = c[5] * y1 + z[2];
    z[2] = c[6] * y1 - c[8] * y + z[3];
    z[3] = c[7] * y1 - c[9] * y;
    return y;
}

// m [4][4], row-major: the state after `steps` samples of zero input is m times the state in front of them.  The filter is
// linear, so the state behind a chunk is (the state reached from rest) + m (the state in front of the chunk).
inline void loudness_transition(const double coef[10], int steps, double m[16]) {
    for (int j = 0; j < 4; j++) {
        double z[4] = {0, 0, 0, 0};
        z[j] = 1.0;
        for (int i = 0; i < steps; i++) loudness_step(coef, 0.0, z);
        for (int i = 0; i < 4; i++) m[4 * i + j] = z[i];
    }
}

// what the kernels take by value: the filter, the transition over kLoudChunk samples, the hop
struct LoudCoef {
    float c[10];
    float m[16];
    int32_t hop;
};

inline LoudCoef loudness_coef(int sample_rate) {
    double c[10], m[16];
    loudness_filter(sample_rate, c);
    loudness_transition(c, kLoudChunk, m);
    LoudCoef k{};
    for (int i = 0; i < 10; i++) k.c[i] = (float)c[i];
    for (int i = 0; i < 16; i++) k.m[i] = (float)m[i];
    k.hop = loudness_hop(sample_rate);
    return k;
}

struct LoudGate {
    double L = -std::numeric_limits<double>::infinity();
    int blocks = 0, abs_pass = 0, rel_pass = 0;
};

// The gates over the blocks of n_rows rows: e holds the rows' sub-block energies back to back, row r has n_sub[r] of them.
// No block straddles two rows; all blocks enter one gating computation.
inline LoudGate loudness_gate(const float *e, const int32_t *n_sub, int n_rows, int hop) {
    LoudGate g;
    std::vector<double> z;
    size_t at = 0;
    for (int r = 0; r < n_rows; r++) {
        for (int j = 0; j + 4 <= n_sub[r]; j++)
            z.push_back(((double)e[at + j] + (double)e[at + j + 1] + (double)e[at + j + 2] + (double)e[at + j + 3]) / (4.0 * hop));
        at += (size_t)(n_sub[r] > 0 ? n_sub[r] : 0);
    }
    g.blocks = (int)z.size();
    auto lufs = [](double v) { return -0.691 + 10.0 * std::log10(v); };  // (log10(0) = -inf: below every gate)
    double sum = 0;
    for (double v : z)
        if (lufs(v) > -70.0) {
            sum += v;
            g.abs_pass++;
        }
    if (g.abs_pass == 0) return g;
    const double gamma = lufs(sum / g.abs_pass) - 10.0;
    sum = 0;
    for (double v : z) {
        const double l = lufs(v);
        if (l > -70.0 && l > gamma) {
            sum += v;
            g.rel_pass++;
        }
    }
    if (g.rel_pass > 0) g.L = lufs(sum / g.rel_pass);
    return g;
}

// the gain of a segment of loudness L and sample peak `peak` (vitsmi.h, "Gain"): in double, rounded once to fp32
inline float level_gain(double L, float peak, const vits_level &t) {
    if (!(L > -std::numeric_limits<double>::infinity())) return 1.0f;  // (-inf, and a NaN from NaN samples: no gain)
    double g = std::pow(10.0, ((double)t.target_lufs - L) / 20.0);
    const double cap = std::pow(10.0, (double)t.max_gain_db / 20.0);
    g = g < cap ? g : cap;
    if (t.peak_ceiling > 0.f && peak > 0.f) {
        const double c = (double)t.peak_ceiling / (double)peak;
        g = g < c ? g : c;
    }
    return (float)g;
}

}  // namespace vitsmi
