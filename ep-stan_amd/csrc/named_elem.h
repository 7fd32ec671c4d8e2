// How one element of a NAMED parameter of the site models is formed from the coordinates of a draw
// theta = [phi | eta (ng) | etb (ng x D)] (site_params.py states the same in NumPy): shared by k_named_moments
// (named_moments.hip) with the order-statistic kernels behind it (quantiles.inc), and k_predict (predict.hip).
#pragma once
#include "epx_device.h"
#include "epx_kernels.h"

namespace epx {

enum { NM_ZERO = 0, NM_ID, NM_EXP, NM_MUL, NM_MULADD };
struct NamedElem {
    int kind;       // ZERO: behind the site's own groups; ID: th[ia]; EXP: exp(th[ia]); MUL: th[ia] * exp(th[ib]);
    int ia, ib, ic; // MULADD: th[ic] + th[ia] * exp(th[ib])
};

// element r of `name` (enum epx_named; its per-site shape flattened in C order) at a site with ng groups;
// model = the b-model id, d = dphi (the Gaussian family's leading log sigma included)
__device__ inline NamedElem named_elem_of(int name, int r, int model, int D, int d, int gauss, int ng) {
    const int o = gauss ? 1 : 0;                         // the Gaussian family's log sigma sits in front of the b-model's phi
    const bool hier = model >= EPX_M4B_SG;               // phi = [mu_a, log sigma_a, mu_b (D), log sigma_b (D)]
    const int lsa = o + (hier ? 1 : 0);                  // log sigma_a
    NamedElem el = {NM_ZERO, 0, 0, 0};
    if (r >= named_len(name, model, D, d, gauss, ng)) return el;              // padding up to the largest site
    switch (name) {
    case EPX_NM_PHI: el.kind = NM_ID; el.ia = r; break;
    case EPX_NM_ETA: el.kind = NM_ID; el.ia = d + r; break;
    case EPX_NM_ALPHA:
        el.kind = hier ? NM_MULADD : NM_MUL; el.ia = d + r; el.ib = lsa; el.ic = o;
        break;
    case EPX_NM_BETA: {
        const int j = r % D;
        el.ia = d + ng + r;
        if (model == EPX_M1B_SG) { el.kind = NM_ID; el.ia = o + 1 + r; }
        else if (model == EPX_M2B_SG) { el.kind = NM_MUL; el.ib = o + 1; }
        else if (model == EPX_M3B_SG) { el.kind = NM_MUL; el.ib = o + 1 + j; }
        else { el.kind = NM_MULADD; el.ib = o + 2 + D + j; el.ic = o + 2 + j; }
        break;
    }
    case EPX_NM_SIGMA_A: el.kind = NM_EXP; el.ia = lsa; break;
    case EPX_NM_ETB: el.kind = NM_ID; el.ia = d + ng + r; break;
    case EPX_NM_SIGMA_B: el.kind = NM_EXP; el.ia = hier ? o + 2 + D + r : o + 1 + r; break;
    case EPX_NM_MU_A: el.kind = NM_ID; el.ia = o; break;
    case EPX_NM_MU_B: el.kind = NM_ID; el.ia = o + 2 + r; break;
    case EPX_NM_SIGMA: el.kind = NM_EXP; el.ia = 0; break;
    default: break;
    }
    return el;
}

__device__ inline double named_value(const NamedElem &el, const double *th) {
    switch (el.kind) {
    case NM_ID: return th[el.ia];
    case NM_EXP: return exp_d(th[el.ia]);
    case NM_MUL: return th[el.ia] * exp_d(th[el.ib]);
    case NM_MULADD: return th[el.ic] + th[el.ia] * exp_d(th[el.ib]);
    default: return 0.0;
    }
}

}  // namespace epx
