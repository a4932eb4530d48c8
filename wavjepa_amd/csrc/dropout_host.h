// Host side of the shared tail wj_dropout_args: p -> (thr, scale), the checks of every _drop entry.
// The _drop entries are compiled only into libwavjepa_hip_dropout.so (-DWJ_DROPOUT_LIB -fvisibility=hidden: the parent entries the shared
// sources also define stay inside that library; common.h's WJ_EXPORT marks what it exports).
#pragma once
#include "../../include/wavjepa_hip_dropout.h"
#include "dropout_pieces.h"

// false: p outside [0, 1) (or NaN)
inline bool drop_params(const wj_dropout_args& a, DropParams& d) {
    if (!(a.p >= 0.f && a.p < 1.f)) return false;
    uint32_t thr = (uint32_t)((double)a.p * 65536.0 + 0.5);    // round(p * 65536) of the fp32 p
    if (thr > 65535u) thr = 65535u;
    d.key0 = (uint32_t)a.seed;
    d.key1 = (uint32_t)(a.seed >> 32);
    d.stream_id = a.stream_id;
    d.call = a.call;
    d.thr = thr;
    d.scale = 65536.0f / (float)(65536u - thr);
    return true;
}
