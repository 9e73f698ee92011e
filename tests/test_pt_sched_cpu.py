"""CPU-only: the host-side decisions both parallel-tempering samplers share (carma_pack_amd/csrc/carma_pt_sched.h: default ladder,
initial proposal factor, length of the next launch, starting-value draws and the search for finite starting values), through the
stand-alone program tests/ptsched/ptsched_main.cpp -- plain C++, no HIP.  The program exits at its first failed check and names
it; it is built and run here WITHOUT sanitizers (a sanitizer build of it is a matter for the command line)."""
import functools
import os
import subprocess

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(os.path.dirname(HERE), "carma_pack_amd", "csrc")
MAIN_SRC = os.path.join(HERE, "ptsched", "ptsched_main.cpp")
MAIN_EXE = os.path.join(HERE, "ptsched", "ptsched_main")
DEPS = [MAIN_SRC, os.path.join(CSRC, "carma_pt_sched.h"), os.path.join(CSRC, "carma_types.h")]
FLAGS = ["-O2", "-std=c++17", "-ffp-contract=off", "-I", CSRC]


@functools.lru_cache(None)
def build_main():
    if not os.path.exists(MAIN_EXE) or any(os.path.getmtime(d) > os.path.getmtime(MAIN_EXE) for d in DEPS):
        subprocess.run(["g++"] + FLAGS + ["-o", MAIN_EXE, MAIN_SRC], check=True, timeout=300)
    return MAIN_EXE


# chunk_sequences: pt_next_chunk on the sequences derived by hand from the three loops it replaced
# chunk_properties: positive chunks that sum to niter; whole thinning intervals, so the sample offset advances by niter / thin
# ladder: T = 1, T = 3 (1, 10, 100), strictly increasing up to T = 64, given temperatures unchanged
# factor_var_rng: initial_factor and pop_var exactly, the first outputs of start_rng
# draws: draw_start within its bounds, and the same key gives the same vector
# starts: find_starts with fake callables (first finite candidate kept, done chains untouched, 4000 rounds, error codes passed up)
@pytest.mark.parametrize("group", ["chunk_sequences", "chunk_properties", "ladder", "factor_var_rng", "draws", "starts"])
def test_pt_sched(group):
    r = subprocess.run([build_main(), group], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    assert "all checks met" in r.stdout


def test_the_header_needs_no_hip():
    """carma_pt_sched.h includes the standard library and carma_types.h only: a plain C++ compiler takes it on its own."""
    r = subprocess.run(["g++", "-std=c++17", "-fsyntax-only", "-Wall", "-x", "c++", os.path.join(CSRC, "carma_pt_sched.h")],
                       capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr[-4000:]
