// What the three kernels of the bridge-sampling evidence estimate share (evidence.hip: k_ev_fit, k_ev_bridge;
// evidence_terms.inc, included by predict.hip: k_ev_terms): a site's own coordinates and the split of its chains.
#pragma once
#include "epx_kernels.h"

namespace epx {

// coordinates of site k (absolute) and its groups
__device__ inline int ev_groups(const EvidenceArgs &a, int k) { return a.site_g0 ? a.site_g0[k + 1] - a.site_g0[k] : 1; }
__device__ inline int ev_coords(const EvidenceArgs &a, int k) { return a.site_g0 ? a.m.d + ev_groups(a, k) * a.pg : a.m.P; }
// draw index (the device's order) of member f of F, of member e of E
__device__ inline int ev_fit_draw(const EvidenceArgs &a, int f) { return (f / a.nh) * a.n + f % a.nh; }
__device__ inline int ev_est_draw(const EvidenceArgs &a, int e) {
    const int ne = a.n - a.nh;
    return (e / ne) * a.n + a.nh + e % ne;
}
__device__ __host__ inline size_t ev_tri(int i, int j) { return (size_t)i * (i + 1) / 2 + j; }

}  // namespace epx
