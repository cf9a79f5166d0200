// mkt_stitch.h -- the host half of read stitching (mkt_stitch.hip): the argument check and the table that carries the one float32
// decision of the definition (include/mkt.h, "read stitching") into the kernels' integer arithmetic.  No HIP in here.
#pragma once
#include <stdint.h>
#include <stdio.h>
#include "../../include/mkt.h"

namespace mkt {

struct StParams {
    uint32_t m, M, phred, cut_tail, min_size;
    float x;
};

// MKT_OK, or MKT_E_ARG with the reason in msg
inline int stitch_check_args(uint32_t m, uint32_t M, double x, uint32_t phred, uint32_t cut_tail, uint32_t min_size, char* msg, size_t cap) {
    if (msg && cap) msg[0] = 0;
    auto say = [&](const char* fmt, unsigned long long a, unsigned long long b2) { if (msg && cap) snprintf(msg, cap, fmt, a, b2); return (int)MKT_E_ARG; };
    if (M > MKT_STITCH_MAX_M) return say("max overlap %llu: above %llu the integer comparison of mismatch densities is no longer the float32 one", M, MKT_STITCH_MAX_M);
    if (m < 1 || m > M) return say("min overlap %llu: need 1 <= min overlap <= max overlap (%llu)", m, M);
    if (!(x >= 0.0 && x <= 1.0)) { if (msg && cap) snprintf(msg, cap, "max mismatch density %g: need 0 .. 1", x); return (int)MKT_E_ARG; }
    if (phred > 127) return say("phred offset %llu: need 0 .. %llu", phred, 127);
    if (cut_tail > 0xFFFFu || min_size > 0xFFFFu) return say("cut tail %llu / min size %llu: need less than 65536", cut_tail, min_size);
    return MKT_OK;
}

// thr[sl], sl = 1 .. M: the largest mm for which float32(mm) / float32(sl) > float32(x) is false (mm = 0 always is: x >= 0)
inline void stitch_thresholds(uint32_t M, float x, uint16_t thr[MKT_STITCH_MAX_M + 1]) {
    thr[0] = 0;
    for (uint32_t sl = 1; sl <= MKT_STITCH_MAX_M; ++sl) {
        uint32_t mm = 0;
        if (sl <= M) while (mm < MKT_STITCH_MAX_READ) { const volatile float d = (float)(mm + 1) / (float)sl; if (d > x) break; ++mm; }
        thr[sl] = (uint16_t)mm;
    }
}

// a string of n characters after deal.flash.pl's substr(s, 0, n - cut): a negative length leaves that many off the end
#ifdef __HIPCC__
__host__ __device__
#endif
inline uint32_t stitch_kept(uint32_t n, uint32_t cut) { return n >= cut ? n - cut : (2 * n > cut ? 2 * n - cut : 0u); }

}  // namespace mkt
