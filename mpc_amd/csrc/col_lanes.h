// col_lanes.h — the column-sliced lane map of the level-walking kernels with the wires in HBM, shared by fused_kernels.hip
// (k_garble_col / k_eval_col: one key per batch) and fused_hbm_keyed_kernels.hip (one key per instance): four lanes per AES
// block, lane J = 4 * (hash lane of the wide form) + column, free lanes behind them.  Device code only; every function is
// inlined.
#pragma once

#include "aes_device.h"
#include "plan.h"

namespace gc {

enum LaneKind { K_NONE = 0, K_AND = 1, K_OR = 2, K_INV = 3, K_FREE = 4 };

__device__ __forceinline__ uint32_t col_pair4(uint32_t v) {  // value of the lane 4 further on (q even) / 4 back (q odd)
    uint32_t r = (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x104, 0xf, 0x5, false);
    return (uint32_t)__builtin_amdgcn_update_dpp((int)r, (int)v, 0x114, 0xf, 0xa, false);
}
__device__ __forceinline__ uint32_t col_whiten(uint32_t xc, uint32_t xc1, uint32_t c, uint32_t tweak, uint32_t k0) {
    const uint32_t kcol = __builtin_amdgcn_alignbit(xc, c == 3 ? 0u : xc1, 31);
    return xor3(kcol, c == 3 ? tweak : 0u, k0);
}
__device__ __forceinline__ uint32_t label_word(const uint4 *label, uint32_t byte_off) {
    return *(const uint32_t *)((const char *)label + byte_off);
}
// lanes of a level in column form (LQA / LQI / LQO: log2 of the wide lanes per AND / INV / OR gate-instance); without HAS_OR
// 0xffffffff: has OR gates
template <int LQA, int LQI, bool HAS_OR = false, int LQO = 0>
__device__ __forceinline__ uint32_t col_lanes(const Step &st, uint32_t ti_log2) {
    if constexpr (!HAS_OR) {
        if (st.n_or) return 0xffffffffu;
        return ((((st.n_and << ti_log2) << LQA) + ((st.n_inv << ti_log2) << LQI)) << 2) + ((st.count - st.nonfree) << ti_log2);
    } else {
        return ((((st.n_and << ti_log2) << LQA) + ((st.n_or << ti_log2) << LQO) + ((st.n_inv << ti_log2) << LQI)) << 2) +
               ((st.count - st.nonfree) << ti_log2);
    }
}
// this lane's place in the column form and its gate's descriptor (fetched before the previous level's barrier)
struct ColPos {
    uint32_t kind, g, inst, q, c;  // kind: K_AND / K_OR (HAS_OR only) / K_INV / K_FREE / K_NONE
};
// HAS_OR: the level's OR gates sit between its AND and its INV gates, as in the gate order of a Step
template <int LQA, int LQI, bool HAS_OR = false, int LQO = 0>
__device__ __forceinline__ ColPos col_classify(const Step &st, uint32_t J, uint32_t ti_log2, uint32_t tim) {
    ColPos p{K_NONE, 0, 0, 0, 0};
    const uint32_t e_and = ((st.n_and << ti_log2) << LQA) << 2;
    if constexpr (!HAS_OR) {
        const uint32_t ncol = e_and + (((st.n_inv << ti_log2) << LQI) << 2);
        if (J < e_and) {
            const uint32_t w = J >> 2;
            p.kind = K_AND, p.c = J & 3u, p.q = w & ((1u << LQA) - 1), p.inst = (w >> LQA) & tim, p.g = w >> (ti_log2 + LQA);
        } else if (J < ncol) {
            const uint32_t w = (J - e_and) >> 2;
            p.kind = K_INV, p.c = J & 3u, p.q = w & ((1u << LQI) - 1), p.inst = (w >> LQI) & tim, p.g = st.n_and + (w >> (ti_log2 + LQI));
        } else if (J - ncol < ((st.count - st.nonfree) << ti_log2)) {
            const uint32_t u = J - ncol;
            p.kind = K_FREE, p.inst = u & tim, p.g = st.nonfree + (u >> ti_log2);
        }
    } else {
        const uint32_t e_or = e_and + (((st.n_or << ti_log2) << LQO) << 2), ncol = e_or + (((st.n_inv << ti_log2) << LQI) << 2);
        if (J < e_and) {
            const uint32_t w = J >> 2;
            p.kind = K_AND, p.c = J & 3u, p.q = w & ((1u << LQA) - 1), p.inst = (w >> LQA) & tim, p.g = w >> (ti_log2 + LQA);
        } else if (J < e_or) {
            const uint32_t w = (J - e_and) >> 2;
            p.kind = K_OR, p.c = J & 3u, p.q = w & ((1u << LQO) - 1), p.inst = (w >> LQO) & tim, p.g = st.n_and + (w >> (ti_log2 + LQO));
        } else if (J < ncol) {
            const uint32_t w = (J - e_or) >> 2;
            p.kind = K_INV, p.c = J & 3u, p.q = w & ((1u << LQI) - 1), p.inst = (w >> LQI) & tim;
            p.g = st.n_and + st.n_or + (w >> (ti_log2 + LQI));
        } else if (J - ncol < ((st.count - st.nonfree) << ti_log2)) {
            const uint32_t u = J - ncol;
            p.kind = K_FREE, p.inst = u & tim, p.g = st.nonfree + (u >> ti_log2);
        }
    }
    return p;
}

}  // namespace gc
