// resample.hpp — the plan of the output-rate resampler (include/vitsmi.h, "Output rate"): L, M, K and the polyphase
// table, computed in double on the host and rounded once to fp32.  Host-side C++17, no HIP types: the plan is a pure
// function of the two rates, answered without a handle or a device.
#pragma once
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <numeric>
#include <string>
#include <vector>

namespace vitsmi {

constexpr int kResampleMaxRate = 384000;
constexpr int64_t kResampleMaxTable = int64_t(1) << 18;  // L * K entries
constexpr int kResampleZ = 16;                           // zero crossings on either side ("kaiser_fast")
constexpr double kResampleBeta = 8.555504641634386;
constexpr double kResampleRolloff = 0.85;

struct ResamplePlan {
    int fi = 0, fo = 0;  // fo == 0: no resampling
    int64_t L = 1, M = 1, K = 0;
    double s = 1.0, W = 0.0;
    bool on() const { return fo != 0; }
    // output samples of n input samples: ceil(n * L / M)
    int64_t count(int64_t n) const { return (n * L + M - 1) / M; }
    // output samples whose K inputs all lie in front of input position P: those with floor(n * M / L) + K / 2 <= P - 1
    int64_t complete(int64_t P) const { return P > K / 2 ? count(P - K / 2) : 0; }
};

// "" or what is wrong with the pair of rates, naming the value
inline std::string resample_plan(int fi, int fo, ResamplePlan &p) {
    char buf[200];
    for (int r : {fi, fo})
        if (r < 1 || r > kResampleMaxRate) {
            std::snprintf(buf, sizeof buf, "sample rate %d outside [1, %d]", r, kResampleMaxRate);
            return buf;
        }
    const int64_t g = std::gcd((int64_t)fi, (int64_t)fo);
    p.fi = fi;
    p.fo = fo;
    p.L = fo / g;
    p.M = fi / g;
    const double ratio = (double)p.L / (double)p.M;
    p.s = kResampleRolloff * (ratio < 1.0 ? ratio : 1.0);
    p.W = kResampleZ / p.s;
    const double half = std::ceil(p.W);
    if (half * 2.0 * (double)p.L > (double)kResampleMaxTable) {
        std::snprintf(buf, sizeof buf, "resampling %d -> %d Hz needs a table of %.0f entries (L = %lld phases x K = %.0f taps); "
                                       "at most %lld are admitted", fi, fo, half * 2.0 * (double)p.L, (long long)p.L, half * 2.0,
                      (long long)kResampleMaxTable);
        return buf;
    }
    p.K = 2 * (int64_t)half;
    return "";
}

// I0(x), the modified Bessel function of order zero: its power series, summed until a term no longer counts
inline double resample_i0(double x) {
    const double q = x * x / 4.0;
    double term = 1.0, sum = 1.0;
    for (int k = 1; k < 500; k++) {
        term *= q / ((double)k * (double)k);
        sum += term;
        if (term < 1e-18 * sum) break;
    }
    return sum;
}

// k(d) = s * sinc(s * d) * kaiser(d / W)
inline double resample_kernel_at(const ResamplePlan &p, double d, double i0_beta) {
    const double kPi = 3.14159265358979323846;
    const double u = d / p.W;
    if (!(std::fabs(u) < 1.0)) return 0.0;
    const double a = kPi * p.s * d;
    const double sinc = a == 0.0 ? 1.0 : std::sin(a) / a;
    return p.s * sinc * resample_i0(kResampleBeta * std::sqrt(1.0 - u * u)) / i0_beta;
}

// h[p][j] = (float)k(p / L + K / 2 - 1 - j), row p at h + p * pitch (pitch >= K; what lies between K and pitch is zeroed)
inline void resample_table(const ResamplePlan &p, float *h, int64_t pitch) {
    const double i0b = resample_i0(kResampleBeta);
    for (int64_t ph = 0; ph < p.L; ph++) {
        float *row = h + ph * pitch;
        for (int64_t j = 0; j < p.K; j++)
            row[j] = (float)resample_kernel_at(p, (double)ph / (double)p.L + (double)(p.K / 2 - 1 - j), i0b);
        for (int64_t j = p.K; j < pitch; j++) row[j] = 0.f;
    }
}

}  // namespace vitsmi
