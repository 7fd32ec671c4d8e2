"""ctypes binding of libepx.so (include/epx.h)."""

import ctypes
import os

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get('EPX_LIB', os.path.join(HERE, 'libepx.so'))   # EPX_LIB: diagnostic builds only

c_double_p = ctypes.POINTER(ctypes.c_double)
c_int64_p = ctypes.POINTER(ctypes.c_int64)
c_int32_p = ctypes.POINTER(ctypes.c_int32)
c_uint8_p = ctypes.POINTER(ctypes.c_uint8)
c_int_p = ctypes.POINTER(ctypes.c_int)
COMM_ID_BYTES = 128          # EPX_COMM_ID_BYTES
OP_SUM, OP_MIN, OP_MAX = 0, 1, 2
# epx_host_allreduce_fn (include/epx.h): int fn(double *buf, long long n, int op, void *user)
HOST_ALLREDUCE_FN = ctypes.CFUNCTYPE(ctypes.c_int, c_double_p, ctypes.c_longlong, ctypes.c_int, ctypes.c_void_p)


class SamplerOpts(ctypes.Structure):
    """epx_sampler_opts (include/epx.h)."""
    _fields_ = [('chains', ctypes.c_int32), ('iter', ctypes.c_int32),
                ('warmup', ctypes.c_int32), ('thin', ctypes.c_int32),
                ('init', ctypes.c_int32), ('max_depth', ctypes.c_int32),
                ('layout', ctypes.c_int32), ('reserved', ctypes.c_int32)]


# every symbol include/epx.h declares, with its argument types
SIGNATURES = {
    'epx_last_error': (ctypes.c_char_p, []),
    'epx_device_count': (ctypes.c_int, [c_int_p]),
    'epx_runtime_info': (ctypes.c_int, [ctypes.c_int, c_int_p, ctypes.c_char_p, ctypes.c_int]),
    'epx_device_synchronize': (ctypes.c_int, [ctypes.c_int]),
    'epx_model_dims': (ctypes.c_int, [ctypes.c_int, ctypes.c_int, c_int_p, c_int_p]),
    'epx_ctx_create': (ctypes.c_int, [ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_int,
                                      c_int64_p, c_double_p, c_int32_p,
                                      ctypes.POINTER(ctypes.c_void_p)]),
    'epx_ctx_create_real': (ctypes.c_int, [ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_int,
                                           c_int64_p, c_double_p, c_double_p,
                                           ctypes.POINTER(ctypes.c_void_p)]),
    'epx_ctx_create_real_groups': (ctypes.c_int, [ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_int,
                                                  c_int64_p, c_int32_p, c_int64_p, c_double_p, c_double_p,
                                                  ctypes.POINTER(ctypes.c_void_p)]),
    'epx_ctx_create_groups': (ctypes.c_int, [ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_int,
                                             c_int64_p, c_int32_p, c_int64_p, c_double_p, c_int32_p,
                                             ctypes.POINTER(ctypes.c_void_p)]),
    'epx_ctx_destroy': (ctypes.c_int, [ctypes.c_void_p]),
    'epx_set_prior': (ctypes.c_int, [ctypes.c_void_p, c_double_p, c_double_p]),
    'epx_set_sites': (ctypes.c_int, [ctypes.c_void_p, ctypes.c_int, c_double_p, c_double_p]),
    'epx_get_sites': (ctypes.c_int, [ctypes.c_void_p, ctypes.c_int, c_double_p, c_double_p]),
    'epx_set_site': (ctypes.c_int, [ctypes.c_void_p, ctypes.c_int, ctypes.c_int, c_double_p, c_double_p]),
    'epx_get_site': (ctypes.c_int, [ctypes.c_void_p, ctypes.c_int, ctypes.c_int, c_double_p, c_double_p]),
    'epx_set_global': (ctypes.c_int, [ctypes.c_void_p, c_double_p, c_double_p]),
    'epx_get_global': (ctypes.c_int, [ctypes.c_void_p, c_double_p, c_double_p]),
    'epx_cavity_batch': (ctypes.c_int, [ctypes.c_void_p, ctypes.c_int, ctypes.c_int, ctypes.c_int, c_uint8_p]),
    'epx_cavity_site': (ctypes.c_int, [ctypes.c_void_p, ctypes.c_int, c_double_p, c_double_p,
                                       c_double_p, c_double_p, c_uint8_p]),
    'epx_get_cavity': (ctypes.c_int, [ctypes.c_void_p, ctypes.c_int, c_double_p, c_double_p]),
    'epx_tilted_batch': (ctypes.c_int, [ctypes.c_void_p, ctypes.c_int, ctypes.c_int, c_int64_p,
                                        ctypes.POINTER(SamplerOpts), ctypes.c_int, c_uint8_p,
                                        c_double_p, c_double_p]),
    'epx_moments_batch': (ctypes.c_int, [ctypes.c_void_p, ctypes.c_int, ctypes.c_int, c_double_p,
                                         ctypes.c_int, ctypes.c_int, c_uint8_p]),
    'epx_set_draw_reuse': (ctypes.c_int, [ctypes.c_void_p, ctypes.c_int]),
    'epx_reweight_batch': (ctypes.c_int, [ctypes.c_void_p, ctypes.c_int, ctypes.c_int, ctypes.c_int, c_double_p,
                                          ctypes.c_int, c_double_p, c_double_p, c_uint8_p, c_double_p, c_double_p]),
    'epx_get_tilted': (ctypes.c_int, [ctypes.c_void_p, ctypes.c_int, c_double_p, c_double_p, c_int_p]),
    'epx_get_draws': (ctypes.c_int, [ctypes.c_void_p, ctypes.c_int, ctypes.c_int, c_double_p]),
    'epx_num_draws': (ctypes.c_int, [ctypes.c_void_p, c_int_p]),
    'epx_site_sums': (ctypes.c_int, [ctypes.c_void_p, c_double_p, ctypes.c_void_p]),
    'epx_packed_len': (ctypes.c_int, [ctypes.c_void_p, c_int_p]),
    'epx_damped_trial': (ctypes.c_int, [ctypes.c_void_p, ctypes.c_double, c_double_p, ctypes.c_void_p,
                                        c_int_p, c_int_p, c_int_p]),
    'epx_accept': (ctypes.c_int, [ctypes.c_void_p, ctypes.c_double]),
    'epx_global_moments': (ctypes.c_int, [ctypes.c_void_p, c_double_p, c_double_p]),
    'epx_force_pd': (ctypes.c_int, [ctypes.c_void_p, ctypes.c_double, ctypes.c_double,
                                    ctypes.c_double, c_uint8_p]),
    'epx_get_adapt': (ctypes.c_int, [ctypes.c_void_p, ctypes.c_int, c_double_p, c_double_p]),
    'epx_logdensity_grad': (ctypes.c_int, [ctypes.c_void_p, ctypes.c_int, c_double_p, c_double_p, c_double_p]),
    'epx_logdensity_grad_layout': (ctypes.c_int, [ctypes.c_void_p, ctypes.c_int, c_double_p, ctypes.c_int,
                                                  ctypes.POINTER(ctypes.c_double), c_double_p]),
    'epx_sample_batch': (ctypes.c_int, [ctypes.c_void_p, ctypes.c_int, ctypes.c_int, c_int64_p,
                                        ctypes.POINTER(SamplerOpts), c_double_p, c_double_p]),
    'epx_nuts_transitions': (ctypes.c_int, [ctypes.c_void_p, ctypes.c_int, ctypes.c_int, c_int64_p,
                                            ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_int,
                                            c_double_p, c_double_p, c_double_p, c_double_p, c_double_p]),
    'epx_last_layout': (ctypes.c_int, [ctypes.c_void_p]),
    'epx_mix_sums': (ctypes.c_int, [ctypes.c_void_p, c_double_p]),
    'epx_named_len': (ctypes.c_int, [ctypes.c_void_p, ctypes.c_int, ctypes.c_int, c_int_p]),
    'epx_named_moments': (ctypes.c_int, [ctypes.c_void_p, ctypes.c_int, ctypes.c_int, c_int32_p, ctypes.c_int,
                                         c_double_p, ctypes.c_int, c_double_p, c_double_p, c_int_p]),
    'epx_named_order_stats': (ctypes.c_int, [ctypes.c_void_p, ctypes.c_int, ctypes.c_int, c_int32_p, ctypes.c_int, c_int64_p,
                                             ctypes.c_int, c_double_p, ctypes.c_int, c_double_p, c_int_p]),
    'epx_pooled_count_pass': (ctypes.c_int, [ctypes.c_void_p, ctypes.c_int, ctypes.c_int, c_int32_p, ctypes.c_int, ctypes.c_int,
                                             ctypes.POINTER(ctypes.c_uint64), ctypes.c_int, c_double_p, ctypes.c_int,
                                             ctypes.POINTER(ctypes.c_longlong), ctypes.POINTER(ctypes.c_longlong),
                                             ctypes.POINTER(ctypes.c_longlong)]),
    'epx_pooled_moments': (ctypes.c_int, [ctypes.c_void_p, ctypes.c_int, ctypes.c_int, c_double_p, c_double_p, ctypes.c_int,
                                          ctypes.c_int, c_double_p, c_double_p, ctypes.POINTER(ctypes.c_longlong)]),
    'epx_predict': (ctypes.c_int, [ctypes.c_void_p, ctypes.c_int, ctypes.c_int, c_int64_p, c_int32_p, c_double_p, c_double_p,
                                   c_double_p, ctypes.c_int, c_double_p, c_int_p]),
    'epx_predict_order_stats': (ctypes.c_int, [ctypes.c_void_p, ctypes.c_int, ctypes.c_int, c_int64_p, c_int32_p, c_double_p,
                                               c_int64_p, ctypes.c_int, ctypes.c_uint64, c_int64_p, ctypes.c_int, c_double_p,
                                               ctypes.c_int, c_double_p, c_int_p]),
    'epx_predict_new_group': (ctypes.c_int, [ctypes.c_void_p, ctypes.c_int, ctypes.c_int, ctypes.c_uint64, ctypes.c_longlong,
                                             ctypes.c_int, ctypes.c_longlong, c_double_p, c_double_p, c_int32_p, ctypes.c_int,
                                             c_int32_p, c_double_p, ctypes.c_int, c_double_p, c_double_p,
                                             ctypes.POINTER(ctypes.c_longlong)]),
    'epx_newgroup_latents': (ctypes.c_int, [ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_uint64, ctypes.c_int32,
                                            ctypes.c_longlong, ctypes.c_longlong, ctypes.c_int, c_double_p]),
    'epx_draw_diagnostics': (ctypes.c_int, [ctypes.c_void_p, ctypes.c_int, ctypes.c_int, c_double_p, ctypes.c_int,
                                            ctypes.c_int, c_double_p, c_int_p]),
    'epx_draw_rank_diagnostics': (ctypes.c_int, [ctypes.c_void_p, ctypes.c_int, ctypes.c_int, c_double_p, ctypes.c_int,
                                                 ctypes.c_int, c_double_p, c_int_p]),
    'epx_rank_normalize': (ctypes.c_int, [ctypes.c_int, ctypes.c_longlong, ctypes.c_int, c_double_p, ctypes.c_int,
                                          c_double_p, c_double_p]),
    'epx_loo': (ctypes.c_int, [ctypes.c_void_p, ctypes.c_int, ctypes.c_int, c_double_p, ctypes.c_int, c_double_p, c_int_p]),
    'epx_psis_rows': (ctypes.c_int, [ctypes.c_int, ctypes.c_longlong, ctypes.c_int, c_double_p, c_double_p]),
    'epx_ppc': (ctypes.c_int, [ctypes.c_void_p, ctypes.c_int, ctypes.c_int, ctypes.c_uint64, ctypes.c_longlong, c_double_p,
                               ctypes.c_int, c_double_p, c_double_p, c_double_p, c_int_p]),
    'epx_site_evidence': (ctypes.c_int, [ctypes.c_void_p, ctypes.c_int, ctypes.c_int, ctypes.c_uint64, ctypes.c_longlong,
                                         c_double_p, ctypes.c_int, ctypes.c_int, c_double_p, c_double_p, c_double_p]),
    'epx_damp_sweep': (ctypes.c_int, [ctypes.c_void_p, ctypes.c_int, c_double_p, c_double_p, ctypes.c_void_p,
                                      c_double_p, c_double_p, ctypes.c_double, c_double_p, c_double_p, ctypes.c_int,
                                      c_double_p]),
    'epx_set_piece_queue': (ctypes.c_int, [ctypes.c_void_p, ctypes.c_int, c_double_p]),
    'epx_set_trace': (ctypes.c_int, [ctypes.c_void_p, ctypes.c_int]),
    'epx_sample_piece': (ctypes.c_int, [ctypes.c_void_p, c_int64_p, ctypes.POINTER(SamplerOpts), ctypes.c_int, c_double_p, c_double_p]),
    'epx_get_trace': (ctypes.c_int, [ctypes.c_void_p, c_double_p, ctypes.c_longlong]),
    'epx_get_team_passes': (ctypes.c_int, [ctypes.c_void_p, ctypes.c_int, ctypes.c_int, c_double_p]),
    'epx_last_segments': (ctypes.c_int, [ctypes.c_void_p]),
    'epx_comm_unique_id': (ctypes.c_int, [ctypes.c_void_p]),
    'epx_comm_init': (ctypes.c_int, [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int, ctypes.c_int]),
    'epx_comm_init_host': (ctypes.c_int, [ctypes.c_void_p, ctypes.c_int, ctypes.c_int, HOST_ALLREDUCE_FN, ctypes.c_void_p]),
    'epx_comm_destroy': (ctypes.c_int, [ctypes.c_void_p]),
    'epx_comm_size': (ctypes.c_int, [ctypes.c_void_p, c_int_p, c_int_p]),
    'epx_comm_allreduce': (ctypes.c_int, [ctypes.c_void_p, c_double_p, ctypes.c_int, ctypes.c_int]),
    'epx_comm_allgather': (ctypes.c_int, [ctypes.c_void_p, c_double_p, ctypes.c_int, c_double_p]),
    'epx_update_trial': (ctypes.c_int, [ctypes.c_void_p, ctypes.c_double, ctypes.c_int, ctypes.c_int,
                                        c_double_p, ctypes.c_int, c_double_p, ctypes.c_int, ctypes.c_int,
                                        c_int_p, c_int_p, c_int64_p, c_double_p, c_double_p]),
    'epx_set_site_order': (ctypes.c_int, [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int]),
    'epx_set_site_split': (ctypes.c_int, [ctypes.c_void_p, ctypes.c_int]),
    'epx_last_split': (ctypes.c_int, [ctypes.c_void_p]),
    'epx_cu_count': (ctypes.c_int, [ctypes.c_void_p]),
    'epx_get_chain_stats': (ctypes.c_int, [ctypes.c_void_p, ctypes.c_int, ctypes.c_int, c_double_p]),
    'epx_rng_probe': (ctypes.c_int, [ctypes.c_int, ctypes.c_uint64, ctypes.c_int, ctypes.c_uint32,
                                     ctypes.c_uint32, ctypes.c_uint32, ctypes.c_uint32, c_double_p]),
    'epx_math_probe': (ctypes.c_int, [ctypes.c_int, ctypes.c_int, ctypes.c_longlong, c_double_p, c_double_p, c_double_p]),
    'epx_invert_normal_params': (ctypes.c_int, [ctypes.c_int, ctypes.c_int, ctypes.c_int, c_double_p,
                                                c_double_p, ctypes.c_int, c_int32_p]),
    'epx_olse': (ctypes.c_int, [ctypes.c_int, ctypes.c_int, ctypes.c_int, c_double_p, ctypes.c_int,
                                c_double_p, c_int32_p]),
}

_lib = None


class EpxError(RuntimeError):
    """An entry point of libepx.so returned an error."""


# The piece hand-off of the default build drops the release fence (csrc/epx_pieces.h): measured behaviour of THIS
# architecture under THIS runtime, litmus-tested there (tests/test_gpu_round4.py).  Anywhere else the loader takes the
# build that keeps the fence.  EPX_LIB overrides (a failing litmus can be answered with EPX_LIB=variants/libepx_fence.so
# at run time, no rebuild); EPX_PIECE_FENCE=1 asks for the fence build by name.
VALIDATED_ARCH, VALIDATED_HIP = 'gfx950', (7, 2)
FENCE_LIB_PATH = os.path.join(os.path.dirname(HERE), 'variants', 'libepx_fence.so')


def _bind(path):
    lib = ctypes.CDLL(path)
    for name, (res, args) in SIGNATURES.items():
        fn = getattr(lib, name)          # AttributeError if a declared symbol is missing
        fn.restype = res
        fn.argtypes = args
    return lib


def runtime_info(lib=None, device=0):
    """((major, minor) of the HIP runtime, gcnArchName of the device) or (None, None) without a device."""
    lib = lib or load()
    n = ctypes.c_int(0)
    if lib.epx_device_count(ctypes.byref(n)) != 0 or n.value < 1:
        return None, None
    if not 0 <= int(device) < n.value:
        device = 0
    v = ctypes.c_int(0)
    buf = ctypes.create_string_buffer(64)
    if lib.epx_runtime_info(int(device), ctypes.byref(v), buf, 64) != 0:
        return None, None
    return (v.value // 10000000, (v.value // 100000) % 100), buf.value.decode()


def load():
    """Load libepx.so; raises (never falls back to a CPU path) when it is missing.
    NOTE: the platform check below initialises the HIP runtime in the calling process when a device is present (it asks
    the rank's own device -- LOCAL_RANK -- for its architecture and runtime version)."""
    global _lib
    if _lib is None:
        import sys
        path = LIB_PATH
        if 'EPX_LIB' not in os.environ and os.environ.get('EPX_PIECE_FENCE', '') == '1':
            if not os.path.exists(FENCE_LIB_PATH):
                raise EpxError('EPX_PIECE_FENCE=1 asks for {} which does not exist: build it with '
                               'ep-stan_amd/csrc/build.sh'.format(FENCE_LIB_PATH))
            path = FENCE_LIB_PATH
        if not os.path.exists(path):
            raise EpxError(
                'libepx.so not found at {}: build it with '
                '`python -c "import __graft_entry__ as g; g.build()"` '
                '(there is no CPU fallback)'.format(path))
        lib = _bind(path)
        if 'EPX_LIB' not in os.environ and path != FENCE_LIB_PATH:
            try:
                dev = int(os.environ.get('LOCAL_RANK', '0'))
            except ValueError:
                dev = 0
            ver, arch = runtime_info(lib, dev)
            if arch is not None and not (arch.startswith(VALIDATED_ARCH) and ver == VALIDATED_HIP):
                # (both libraries hold gfx950 code only -- build.sh -- so what this branch really covers is another HIP
                # runtime on gfx950; on another architecture neither loads a kernel)
                if os.path.exists(FENCE_LIB_PATH):
                    print('epstan_amd: %s / HIP %s is not the platform the fence-free piece hand-off was validated on (%s / HIP %d.%d): '
                          'loading %s' % (arch, ver, VALIDATED_ARCH, VALIDATED_HIP[0], VALIDATED_HIP[1], FENCE_LIB_PATH), file=sys.stderr)
                    lib = _bind(FENCE_LIB_PATH)
                else:
                    print('epstan_amd: WARNING: %s / HIP %s is not the platform the fence-free piece hand-off was validated on '
                          '(%s / HIP %d.%d) and %s is missing: keeping the fence-free build; pieced launches (epx_set_piece_queue) '
                          'are not validated here' % (arch, ver, VALIDATED_ARCH, VALIDATED_HIP[0], VALIDATED_HIP[1], FENCE_LIB_PATH),
                          file=sys.stderr)
        _lib = lib
    return _lib


def check(rc):
    if rc != 0:
        raise EpxError(load().epx_last_error().decode('utf-8', 'replace'))


def dptr(a):
    """double* of a float64 array (None -> NULL)."""
    if a is None:
        return None
    assert a.dtype == np.float64
    return a.ctypes.data_as(c_double_p)


# enum epx_math_probe_kind (include/epx.h), in its order
MATH_PROBE_KINDS = ('rcp', 'exp', 'exp_vc', 'log1p_unit', 'log_ge1', 'log_ge1_vc', 'log_pos', 'lse2_lean', 'lse2', 'merge',
                    'terms', 'split', 'split2_a', 'split2_b', 'pair_lean_a', 'pair_lean_b')


def math_probe(kind, a, b=None, device=0):
    """TEST HOOK epx_math_probe: the (n, 4) results of the lean device function `kind` (a name of MATH_PROBE_KINDS) at
    (a[i], b[i]); b defaults to zeros."""
    a = np.ascontiguousarray(a, dtype=np.float64)
    b = np.zeros_like(a) if b is None else np.ascontiguousarray(b, dtype=np.float64)
    assert a.ndim == 1 and a.shape == b.shape
    out = np.zeros((a.shape[0], 4))
    check(load().epx_math_probe(int(device), MATH_PROBE_KINDS.index(kind), a.shape[0], dptr(a), dptr(b), dptr(out)))
    return out


def device_synchronize(device=0):
    check(load().epx_device_synchronize(int(device)))


def device_count():
    n = ctypes.c_int(0)
    rc = load().epx_device_count(ctypes.byref(n))
    return n.value if rc == 0 else 0
