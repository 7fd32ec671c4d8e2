// The scalars of one chain with their start values: the scope that nuts_state_machine.inc runs in, textually
// included once per kernel body (k_nuts and k_nuts_spec's bookkeeping wave in nuts.hip, duo_piece in nuts_duo.hip,
// stream_piece in nuts_stream.hip) in front of the chain's loop.
//
// Declares, in this order (the order of the declarations is the order of the kernel's loop-carried values, and the
// register allocation of the sampler kernels follows it: keep it):
//   once-per-transition scalars, `double` unless the includer keeps them elsewhere (see EPX_CHAIN_SCALARS_BOUND):
//       lps plp mlp b_plp lsw                           log densities (sample, tree ends, proposal), log sum of weights
//       da_mu s_bar x_bar da_count va_n                 dual averaging, Welford count
//       eps_sum acc_sum depth_sum nleap_tot             statistics of the run
//   double zlp eps_l                                    log density of the state just evaluated, signed step of the next
//                                                       leapfrog (0: evaluate only); see EPX_CHAIN_HEAD_DECLARED
//   double b_key eps ngrad H0 sum_metro u_dir gum dhb lw_m lw_s
//   const double DELTA GAMMA T0 KAPPA LOG08             Stan's adaptation constants (stepsize_adaptation.hpp @ 2.17)
//   int    va_init_buf va_term va_base va_counter va_wsize va_next          warm-up windows (windowed_adaptation.hpp)
//          ndiv npost kept failed
//          t mode depth leaf nleaf fwd nleap divergent init_try ss_trial ss_dir ss_after_update
//   uint32_t ss_t
// Expects in scope: `a` (the kernel's arguments).
// EPX_CHAIN_SCALARS_BOUND: the includer has declared the fourteen once-per-transition scalars itself, behind the
// interface of GScal / RScal (nuts_common.h), bound them to their storage and set FIVE of them to 0 there -- lps, plp,
// mlp, b_plp, lsw: exactly the names under EPX_CS_ZERO below (in a global store the order of the stores is part of the
// kernel's schedule) -- while the other nine, the names under EPX_CS_START, get their start values here.  Whoever adds
// a scalar of that kind adds it to the includer's declaration and binding, and to ONE of the two groups.
// EPX_CHAIN_HEAD_DECLARED: lps, zlp, plp, mlp, b_key, b_plp and eps_l exist already.  k_nuts_spec: its gradient waves use
// zlp and eps_l, too, and its bookkeeping wave keeps the five others declared in front of its vectors' start values --
// declared behind them, (b_key, b_plp) get each other's registers (profiles/chain_scaffolding_identity.txt).
#ifndef EPX_CHAIN_SCALARS_BOUND
#define EPX_CS_ZERO(x_) double x_ = 0
#define EPX_CS_START(x_, v_) double x_ = v_
#else
#define EPX_CS_ZERO(x_) (void)0
#define EPX_CS_START(x_, v_) x_ = v_
#endif
#ifndef EPX_CHAIN_HEAD_DECLARED
    EPX_CS_ZERO(lps);
    double zlp = 0;
    EPX_CS_ZERO(plp); EPX_CS_ZERO(mlp);
    double b_key = 0;
    EPX_CS_ZERO(b_plp);
#endif
    // adaptation state (stepsize_adaptation.hpp / windowed_adaptation.hpp @ Stan 2.17)
    const double DELTA = 0.8, GAMMA = 0.05, T0 = 10.0, KAPPA = 0.75, LOG08 = -0.2231435513142097558;
    double eps = 1.0;
    EPX_CS_START(da_mu, log(10.0)); EPX_CS_START(s_bar, 0.0); EPX_CS_START(x_bar, 0.0); EPX_CS_START(da_count, 0.0);
    int va_init_buf = 75, va_term = 50, va_base = 25;           // initial fast buffer, terminal buffer, first slow window ...
    if (va_init_buf + va_base + va_term > a.warmup && a.warmup >= 20) {         // ... rescaled to a short warm-up
        va_init_buf = (int)(0.15 * a.warmup);
        va_term = (int)(0.1 * a.warmup);
        va_base = a.warmup - (va_init_buf + va_term);
    }
    int va_counter = 0, va_wsize = va_base, va_next = va_init_buf + va_base - 1;
    EPX_CS_START(va_n, 0.0);
    // statistics
    EPX_CS_START(eps_sum, 0.0); EPX_CS_START(acc_sum, 0.0); EPX_CS_START(depth_sum, 0.0); EPX_CS_START(nleap_tot, 0.0);
    double ngrad = 0;
    int ndiv = 0, npost = 0, kept = 0, failed = 0;
    // transition state
    int t = 0, mode = MODE_INIT, depth = 0, leaf = 0, nleaf = 1, fwd = 1, nleap = 0, divergent = 0, init_try = 0;
    int ss_trial = 0, ss_dir = 0, ss_after_update = 0;
    uint32_t ss_t = 0;
    double H0 = 0;
    EPX_CS_ZERO(lsw);
    double sum_metro = 0;
#ifndef EPX_CHAIN_HEAD_DECLARED
    double eps_l = 0;
#endif
    // Batched random numbers: lane x of u_dir holds DIR(depth x) for x < 16 and TOP(depth x-16)
    // for 16 <= x < 32 of the current transition; lane x of gum holds the Gumbel variate
    // -log(-log u) of leaf (leaf & ~63) + x of the current doubling.
    double u_dir = 0.0, gum = 0.0;
    // Leaf energy errors dH of the current doubling, lane (leaf & 63); reduced 64 at a time (flush_leaf_dh) into
    // the running log-sum-weight (lw_m + log lw_s) and the accept statistic.
    double dhb = 0.0, lw_m = -INFINITY, lw_s = 0.0;
#undef EPX_CS_ZERO
#undef EPX_CS_START
