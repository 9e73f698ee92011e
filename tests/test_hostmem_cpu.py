"""CPU-only: the owners of device and pinned buffers (carma_pack_amd/csrc/carma_devbuf.h: DevMem, DevBuf, PinnedBuf), the buffer
requests of the sampler states (carma_pt_state.h) and the model-row packers (carma_model_pack.h: normalize_roots, pack_model_row,
pack_model_single) of the host layer, through the stand-alone program tests/hostmem/hostmem_main.cpp.  The program brings its own
carma_dev_malloc / carma_dev_free and carma_pinned_malloc / carma_pinned_free over malloc / free, which record every request and
release and can fail a request: it needs the HIP headers and no HIP runtime.  It exits at its first failed
check and names it; it is built and run here WITHOUT sanitizers (a sanitizer build of it is a matter for the command line)."""
import functools
import os
import subprocess

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
CSRC = os.path.join(ROOT, "carma_pack_amd", "csrc")
MAIN_SRC = os.path.join(HERE, "hostmem", "hostmem_main.cpp")
MAIN_EXE = os.path.join(HERE, "hostmem", "hostmem_main")
DEPS = [MAIN_SRC, os.path.join(CSRC, "carma_devbuf.h"), os.path.join(CSRC, "carma_model_pack.h"),
        os.path.join(CSRC, "carma_pt_state.h"), os.path.join(CSRC, "carma_mseries_plan.h"), os.path.join(CSRC, "carma_smooth_plan.h"),
        os.path.join(ROOT, "include", "carma_mi355.h")]
FLAGS = ["-O2", "-std=c++17", "-D__HIP_PLATFORM_AMD__", "-I/opt/rocm/include", "-I", CSRC]


@functools.lru_cache(None)
def build_main():
    if not os.path.exists(MAIN_EXE) or any(os.path.getmtime(d) > os.path.getmtime(MAIN_EXE) for d in DEPS):
        subprocess.run(["g++"] + FLAGS + ["-o", MAIN_EXE, MAIN_SRC], check=True, timeout=300)
    return MAIN_EXE


# devmem_alloc: exact sizes, release on re-allocation / destruction / release(), moves, a failed request leaves it empty
# devmem_need: the growth rule max(bytes + bytes / 4, 4096) on the sequence 1, 4096, 4097, 5000, 10000, 100; failed growth
# roots: normalize_roots for p = 1 ... 7 against orders written out by hand; open sets are CARMA_EINVAL
# rows: pack_model_row / pack_model_single for p = 2, 3, 7 against hand-written rows (zero padding, pre-filled rows, open roots)
# typed_buf / pinned_buf: DevBuf<T> / PinnedBuf<T>: bytes = count * sizeof(T), conversion to T*, arithmetic, moves, empty after a
# failed request, each over its own pair of entry points
# ensemble: the requests of a create of the ladder, row, lane and multi-series states, in bytes and order; every one of them failed in
# turn: the failure is reported, deleting the state leaves nothing live and releases nothing twice
# samples: 8, 3, 20 samples per ladder are two pairs of requests of R ns d 8 and R ns 8 bytes; a failed request of a pair leaves
# capacity 0 and no buffer, the next reserve asks for both
# boundary: each of the four boundary buffers of the sharded ladder failed in turn leaves none; the next reserve asks for all four
# bind: caller-owned chain state releases the library's two buffers once and never reaches the allocator, also when the state goes
@pytest.mark.parametrize("group", ["devmem_alloc", "devmem_need", "roots", "rows", "typed_buf", "pinned_buf", "ensemble", "samples",
                                   "boundary", "bind"])
def test_hostmem(group):
    r = subprocess.run([build_main(), group], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    assert "all checks met" in r.stdout


def test_the_header_needs_no_hip():
    """carma_model_pack.h includes the standard library and include/carma_mi355.h only: a plain C++ compiler takes it on its
    own, without the HIP include path."""
    r = subprocess.run(["g++", "-std=c++17", "-fsyntax-only", "-Wall", "-x", "c++", os.path.join(CSRC, "carma_model_pack.h")],
                       capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr[-4000:]
