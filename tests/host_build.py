"""TEST INFRASTRUCTURE: build the host-compiled doubles of device code (tests/host/*.cpp) with g++.

``build_host_library(name, sources)`` -> ctypes library of ``sources[0]``, cached per hash of the
sources under the system temp directory; every loader of a host double goes through it.
``lssmm_host()`` -> the library exporting the vmp_lssmm_* C ABI, compiled from the very header the
HIP kernels include (bayespy_amd/csrc/vmp_lssmm_dev.h) plus the host+device special functions
sliced out of vmp_common.h."""
import ctypes
import functools
import hashlib
import os
import subprocess
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, 'bayespy_amd', 'csrc')
FLAGS = ['-O2', '-std=c++17', '-shared', '-fPIC', '-ffp-contract=off']


def special_functions_text():
    text = open(os.path.join(CSRC, 'vmp_common.h')).read()
    s = text.index('__host__ __device__ inline double vmp_digamma')
    e = text.index('#ifdef __HIPCC__')
    return '#include <math.h>\n#define __host__\n#define __device__\n' + text[s:e] + \
        '\n#undef __host__\n#undef __device__\n'


def build_host_library(name, sources, flags=(), prelude=None):
    """``sources``: paths below the repository root; the first is compiled, the others are the
    headers it includes (they only enter the hash).  ``prelude``: text included ahead of it."""
    srcs = [os.path.join(ROOT, p) for p in sources]
    h = hashlib.sha256(' '.join(flags).encode() + (prelude or '').encode())
    for p in srcs:
        with open(p, 'rb') as f:
            h.update(f.read())
    d = os.path.join(tempfile.gettempdir(), 'bayespy_amd_%s_%s' % (name, h.hexdigest()[:16]))
    so = os.path.join(d, 'lib%s_host.so' % name)
    if not os.path.exists(so):
        os.makedirs(d, exist_ok=True)
        # per-process names + atomic renames: several pytest workers may build at once
        tmp = so + '.%d.tmp' % os.getpid()
        cmd = ['g++'] + FLAGS + list(flags)
        if prelude is not None:
            pre = os.path.join(d, 'prelude.%d.h' % os.getpid())
            with open(pre, 'w') as f:
                f.write(prelude)
            cmd += ['-include', pre]
        subprocess.check_call(cmd + [srcs[0], '-o', tmp])
        os.replace(tmp, so)
    return ctypes.CDLL(so)


@functools.lru_cache(None)
def lssmm_host():
    return build_host_library('lssmm', ['tests/host/lssmm_host.cpp',
                                        'bayespy_amd/csrc/vmp_lssmm_dev.h', 'include/vmp_hip.h'],
                              flags=('-pthread',), prelude=special_functions_text())
