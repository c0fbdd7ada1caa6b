// What the trim, loudness and shape drivers add to their own hand-stated walks: the ONE walk of a delivery call
// (workspace.hpp, carve_delivery_call) against the carve_* sequence written out here, buffer by buffer - levelled or not,
// shaped or not (0 and 5 knots), with and without the scan's slots, behind its own delivery buffers and behind a resampled
// waveform's.  No memory is touched: both walks run over a base that is only a number.
#pragma once
#include <cstdint>

#include "workspace.hpp"

namespace vitsmi {

inline bool delivery_call_walk_agrees(int B, int S) {
    char *const base = reinterpret_cast<char *>(uintptr_t(1) << 44);
    const size_t cap = size_t(1) << 40;
    const int K = 33;  // (a resampler's taps: any)
    bool ok = true;
    for (int v = 0; v < 32; v++) {
        const bool resampled = v & 1, scan = v & 2, lev = v & 4, shaped = v & 8;
        const int64_t n_knots = v & 16 ? 5 : 0;
        Carver hand(base, cap), one(base, cap);
        DeliveryCallBufs want{};
        want.dlv = resampled ? carve_resample(hand, B, S, K).dlv : carve_delivery(hand, B, S);
        if (scan) {
            want.trim = carve_trim(hand, B);
            if (lev) want.level = carve_level(hand, B, S);
            if (shaped) want.shape = carve_shape(hand, B, n_knots);
        }
        const DeliveryNeeds need{scan, lev, shaped, n_knots};
        DeliveryCallBufs got{};
        if (resampled) {
            const DeliveryBufs front = carve_resample(one, B, S, K).dlv;
            got = carve_delivery_call(one, B, S, need, &front);
        } else
            got = carve_delivery_call(one, B, S, need);
        const size_t dry = carved_bytes([&](Carver &cv) {
            if (resampled) carve_resample(cv, B, S, K);
            carve_delivery_call(cv, B, S, need, resampled ? &want.dlv : nullptr);
        });
        ok = ok && one.fits() && one.used == hand.used && dry == hand.used && got.dlv.packed == want.dlv.packed &&
             got.dlv.segs == want.dlv.segs && got.dlv.peak == want.dlv.peak && got.trim.bounds == want.trim.bounds &&
             got.trim.peak_all == want.trim.peak_all && got.level.segs == want.level.segs && got.level.fin == want.level.fin &&
             got.level.init == want.level.init && got.level.part == want.level.part && got.level.result == want.level.result &&
             got.level.n_peaks == want.level.n_peaks && got.level.n_chunks == want.level.n_chunks &&
             got.level.n_subs == want.level.n_subs && got.shape.segs == want.shape.segs && got.shape.knots == want.shape.knots;
    }
    return ok;
}

}  // namespace vitsmi
