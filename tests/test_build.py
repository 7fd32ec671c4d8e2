"""The build of libepx (ep-stan_amd/csrc/Makefile): one statement of the library's translation units, header dependencies
from the compiler, and variants that are whole libraries.  CPU only; runs after build()."""
import ctypes
import glob
import os
import re
import shutil
import subprocess

import pytest

from epstan_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, 'ep-stan_amd', 'csrc')
VARIANTS = os.path.join(ROOT, 'variants')
FENCE_TUS = {'nuts_duo', 'nuts_stream'}
# every .h and .inc of csrc/ and the C ABI's header, named as the sources name them (relative to csrc/)
HEADERS = sorted(os.path.basename(p) for p in glob.glob(os.path.join(CSRC, '*.h')) + glob.glob(os.path.join(CSRC, '*.inc'))) \
    + ['../../include/epx.h']


def make(*args, env=None):
    """Runs make in csrc/ (skips without hipcc); returns the CompletedProcess."""
    hipcc = os.environ.get('HIPCC') or shutil.which('hipcc') or '/opt/rocm/bin/hipcc'
    if not os.path.exists(hipcc):
        pytest.skip('no hipcc')
    e = dict(os.environ, HIPCC=hipcc)
    e.pop('MAKEFLAGS', None)
    e.update(env or {})
    return subprocess.run(['make', '-C', CSRC, '--no-print-directory'] + list(args), env=e, stdout=subprocess.PIPE,
                          stderr=subprocess.STDOUT, universal_newlines=True)


def compiled(out):
    """The objects that the compile commands of a make -n listing write."""
    return sorted(re.search(r' -o (\S+)', l).group(1) for l in out.splitlines() if ' -c ' in l)


def linked(out):
    """{library: [objects]} of the link commands of a make -n listing."""
    return {re.search(r' -o (\S+)', l).group(1): re.findall(r'\S+\.o\b', l) for l in out.splitlines() if ' -shared ' in l}


def include_closure(tu):
    """Every file that <tu>.hip reaches through #include "...", relative to csrc/ (found by scanning the sources)."""
    seen, todo = set(), [tu + '.hip']
    while todo:
        f = todo.pop()
        for inc in re.findall(r'^\s*#\s*include\s+"([^"]+)"', open(os.path.join(CSRC, f)).read(), re.M):
            inc = os.path.normpath(os.path.join(os.path.dirname(f), inc))
            if inc not in seen:
                seen.add(inc)
                todo.append(inc)
    return seen


def default_link():
    libs = linked(make('-n', '-B', '../libepx.so').stdout)
    assert list(libs) == ['../libepx.so'], libs
    return libs['../libepx.so']


def test_build_is_idempotent():
    """After build() nothing is out of date."""
    r = make('-q')
    assert r.returncode == 0, r.stdout


@pytest.mark.parametrize('header', HEADERS)
def test_header_rebuilds_exactly_its_includers(header):
    """A newer header (make -W: nothing is touched) recompiles the translation units that include it, directly or not, in
    build/ and -- the two with the piece hand-off -- in build_fence/, no other, and relinks both libraries."""
    tus = [os.path.basename(p)[:-4] for p in glob.glob(os.path.join(CSRC, '*.hip'))]
    users = {t for t in tus if header in include_closure(t)}
    assert users, 'no translation unit includes %s' % header
    if header == 'named_elem.h':
        assert users == {'named_moments', 'predict'}
    if header == 'epx_stream_tile.h':
        assert users == {'nuts_stream'}
    r = make('-n', '-W', header)
    assert r.returncode == 0, r.stdout
    want = ['build/%s.o' % t for t in users] + ['build_fence/%s.o' % t for t in users & FENCE_TUS]
    assert compiled(r.stdout) == sorted(want), r.stdout
    assert sorted(linked(r.stdout)) == ['../../variants/libepx_fence.so', '../libepx.so'], r.stdout


def resolves_every_symbol(path):
    lib = ctypes.CDLL(path)                        # (RTLD_NOW: an object missing from the link line fails here)
    return [name for name in _lib.SIGNATURES if not hasattr(lib, name)]


def test_variant_is_a_whole_library():
    """make variant recompiles the named translation unit and links it with EVERY other object of the library."""
    lib, objdir = os.path.join(VARIANTS, 'libepx_pytest_probe.so'), os.path.join(CSRC, 'build_var', 'pytest_probe')
    try:
        r = make('variant', 'NAME=pytest_probe', 'TUS=named_moments', 'EXTRA=-DEPX_VARIANT_PROBE')
        assert r.returncode == 0, r.stdout
        assert resolves_every_symbol(lib) == []
        assert resolves_every_symbol(os.path.join(VARIANTS, 'libepx_fence.so')) == []
    finally:
        shutil.rmtree(objdir, ignore_errors=True)
        if os.path.exists(lib):
            os.remove(lib)


@pytest.mark.parametrize('script', ['build_variant.sh', 'build_stream_variant.sh', 'schedule_robustness.sh'])
def test_helper_links_the_librarys_own_object_list(script):
    """What a scripts/ helper would link (MAKEFLAGS=n: nothing is built) is one object per translation unit of libepx.so."""
    want = sorted(os.path.basename(o) for o in default_link())
    assert len(want) == len(set(want)) >= 9
    e = dict(os.environ, MAKEFLAGS='n')
    r = subprocess.run([os.path.join(ROOT, 'scripts', script), 'pytest_dummy', '-DEPX_VARIANT_PROBE'], env=e,
                       stdout=subprocess.PIPE, stderr=subprocess.STDOUT, universal_newlines=True)
    assert r.returncode == 0, r.stdout
    libs = linked(r.stdout)
    assert len(libs) == 1 and re.fullmatch(r'\.\./\.\./variants/libepx_(sched_)?pytest_dummy\.so', list(libs)[0]), r.stdout
    assert sorted(os.path.basename(o) for o in list(libs.values())[0]) == want, r.stdout
    assert not os.path.exists(os.path.join(CSRC, 'build_var', 'pytest_dummy'))


def test_failed_compile_links_nothing():
    lib, objdir = os.path.join(VARIANTS, 'libepx_pytest_bad.so'), os.path.join(CSRC, 'build_var', 'pytest_bad')
    try:
        r = make('variant', 'NAME=pytest_bad', 'TUS=named_moments', 'EXTRA=-include /nonexistent.h')
        assert r.returncode != 0, r.stdout
        assert 'nonexistent.h' in r.stdout
        assert not os.path.exists(lib)
    finally:
        shutil.rmtree(objdir, ignore_errors=True)
        if os.path.exists(lib):
            os.remove(lib)
