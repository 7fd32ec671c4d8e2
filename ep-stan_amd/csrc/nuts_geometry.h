// Sampler geometry: the sizes of the records the resident sampler kernels keep in LDS and the thread counts of their
// workgroups, each written ONCE.  The kernels (nuts.hip, nuts_duo.hip, nuts_gradient_groups.inc) initialise their
// constexpr names from these functions, the host's layout functions (nuts_lds_layout, nuts_duo_lds_layout) and the
// launchers call the same ones: a record changes in one line here.  Plain constexpr functions are host and device code
// alike under hip-clang, and a kernel's constexpr name initialised from one compiles to the code of the literal
// (profiles/lds_geometry_identity.txt).  Sizes are in doubles unless the name says bytes.
#pragma once
#include <stddef.h>

namespace epx {

// LDS of a gfx950 CU, all of which one workgroup may have
constexpr size_t lds_capacity() { return 160 * 1024; }

// doubles per level of a chain's tree stack: (rho, p_sharp of the left end) of a pending left sibling
constexpr int nuts_stack_record(int nv) { return 2 * nv * 64; }

// ------------------------------------------------------------------ resident kernels (nuts.hip: k_nuts, k_nuts_spec)
// XREC, per-wave exchange record of a leapfrog: the wave's partial X'g (64), its partial Omega product (nv x 64), sum g, log-lik
constexpr int nuts_exchange_record(int nv) { return 64 * (1 + nv) + 2; }
// k_nuts_spec, MREC, mailbox entry of the gradient waves: q, p, grad, ll, -, generation, -, per-lane lp terms
constexpr int nuts_spec_mail_record(int nv) { return 3 * nv * 64 + 4 + 64; }
// k_nuts_spec, CREC, control record of the bookkeeping wave: q, p, grad, metric, eps_l, command, stamp
constexpr int nuts_spec_control_record(int nv) { return 4 * nv * 64 + 4; }
// k_nuts_spec: four gradient waves and the bookkeeping wave
constexpr int nuts_spec_threads() { return 64 * (4 + 1); }
// several groups per site (nuts_gradient_groups.inc): GREC, per-group record (dbeta (64), dalpha, -) ...
constexpr int nuts_group_record() { return 66; }
// ... WREC, per-wave record (Omega partials (nv x 64), ll, -) ...
constexpr int nuts_wave_record(int nv) { return 64 * nv + 2; }
// ... and what one leapfrog parity holds of them: wpc wave records, then ngmax group records
constexpr int nuts_group_exchange(int nv, int wpc, int ngmax) { return wpc * nuts_wave_record(nv) + ngmax * nuts_group_record(); }
// the site's ngmax + 1 group row limits (ints) in front of qcopy, in whole 16-byte pairs
constexpr int nuts_group_limit_doubles(int ngmax) { return ((ngmax + 1 + 3) / 4) * 2; }

// ------------------------------------------------------------------ row-wave / state-wave kernels (nuts_duo.hip: duo_piece)
// TEAM (layout 7): the four row waves serve the four chains of the site together, in lock step
constexpr bool duo_team(int cpb, int rw) { return cpb == 4 && rw == 4; }
// BKW (layout 6): one chain per workgroup, whose bookkeeping and cavity term have waves of their own
constexpr bool duo_bkw(int cpb) { return cpb == 1; }
// threads of a workgroup: TEAM four state + four row waves; else per chain a state wave + rw row waves, BKW two waves more
constexpr int duo_threads(int cpb, int rw) { return 64 * (duo_team(cpb, rw) ? 8 : cpb * (1 + rw) + (duo_bkw(cpb) ? 2 : 0)); }
// RES, result of a row wave: X'g (dp), sum g, log-lik (the job, (alpha, beta), takes as much at the head of the slot)
constexpr int duo_res(int dp) { return dp + 2; }
// VN, the v = phi - mu and the Omega v line: TEAM keeps only the d <= 2 dp + 2 live ones, in whole 16-byte pairs
constexpr int duo_vn(int nv, int dp, int cpb, int rw) { return (duo_team(cpb, rw) && 2 * dp + 8 < nv * 64) ? 2 * dp + 8 : nv * 64; }
// a chain's slot with rw > 1: [job RES | v VN | per row wave a result RES | Omega v VN] -- VOFF, RESO, OVOFF are where
// the last three begin; with rw == 1 the slot is the job / result record alone
constexpr int duo_voff(int dp) { return duo_res(dp); }
constexpr int duo_reso(int nv, int dp, int cpb, int rw) { return duo_voff(dp) + duo_vn(nv, dp, cpb, rw); }
constexpr int duo_ovoff(int nv, int dp, int cpb, int rw) { return duo_reso(nv, dp, cpb, rw) + rw * duo_res(dp); }
constexpr int duo_slot_doubles(int nv, int dp, int cpb, int rw) {
    return rw == 1 ? duo_res(dp) : duo_ovoff(nv, dp, cpb, rw) + duo_vn(nv, dp, cpb, rw);
}
// NFLAG, hand-off words per chain: job, one per row wave's results, BKW: mail, acknowledged, control generation, cavity term;
// TEAM: the job word alone
constexpr int duo_nflag(int cpb, int rw) { return duo_team(cpb, rw) ? 1 : 1 + rw + (duo_bkw(cpb) ? 4 : 0); }
// bytes of the workgroup's flag block; TEAM: cpb job words, cpb result words and the live-chain word, in whole 16 bytes (48)
constexpr int duo_flag_bytes(int cpb, int rw) { return duo_team(cpb, rw) ? ((2 * cpb + 1) * 4 + 15) & ~15 : cpb * duo_nflag(cpb, rw) * 4; }
// BKW, MREC, mailbox entry: q, p, grad, per-element log-density terms; ll, -, generation, -
constexpr int duo_mail_record(int nv) { return 4 * nv * 64 + 4; }
// BKW, CREC, control record: q, p, grad, metric, eps_l, command
constexpr int duo_control_record(int nv) { return 4 * nv * 64 + 4; }
// OU: the cavity precision in LDS is zero padded to whole groups of this many column pairs, one round of the mat-vec
constexpr int duo_ou(int nv) { return nv > 1 ? 4 : 8; }

}  // namespace epx
