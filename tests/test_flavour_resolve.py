"""Which compiled sweep_fast_kernel a class launch gets (mvtopicmodel_amd/csrc/mvhdp_flavour.h), without a GPU: the header's rule,
compiled here with the host compiler, against the table recorded from the two if-ladders it replaced
(tests/golden/fast_flavour_table.txt), and the rule's range against the header's list of the instantiations that exist."""
import ctypes as C
import itertools
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TABLE = os.path.join(ROOT, "tests", "golden", "fast_flavour_table.txt")
# rounds, K, debug, walk, narrow, live_rows, live16, mix, counts12
DOMAIN = [(1, 2, 4, 8, 16), (511, 512, 513, 1024, 1025), (0, 1), (0, 1), (0, 1, 2), (0, 1), (0, 1), (0, 1), (0, 1)]
# Compiled and never asked for: the two-batch live-rows flavour of the 2-round variant on the mirror without ROOMY.  Two-batch rows are
# K in 513 .. 1024, and from K = 512 on the 2-round variant on the mirror is the ROOMY build (which has that flavour of its own).
NEVER_RESOLVED = {(2, 0, 1, 1, 0, 2, 0)}

SHIM = r"""
#include "mvhdp_flavour.h"
static void put(const FastFlavour& f, int* o) { o[0] = f.rmax; o[1] = f.debug; o[2] = f.walk; o[3] = f.narrow; o[4] = f.roomy; o[5] = f.liverows; o[6] = f.mix; }
extern "C" {
int flavour_resolve(const int* q, int* out)
{
    FastFlavour f;
    if (!mvhdp_fast_resolve(FastRequest{q[0], q[1], q[2] != 0, q[3] != 0, q[4], q[5] != 0, q[6] != 0, q[7] != 0, q[8] != 0}, &f)) return 0;
    put(f, out);
    return 1;
}
int flavour_count(void) { return MVHDP_N_FAST_FLAVOURS; }
void flavour_key(int i, int* out) { put(mvhdp_fast_flavours[i], out); }
int slim_max_rounds(void) { return MVHDP_SLIM_MAX_ROUNDS; }
}
"""


@pytest.fixture(scope="module")
def shim(tmp_path_factory):
    cxx = shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
    if cxx is None:
        pytest.fail("no host C++ compiler: the flavour header cannot be checked")
    d = tmp_path_factory.mktemp("flavour")
    src, lib = d / "flavour_shim.cpp", d / "libflavour_shim.so"
    src.write_text(SHIM)
    subprocess.check_call([cxx, "-std=c++17", "-O1", "-Wall", "-Werror", "-shared", "-fPIC",
                           "-I", os.path.join(ROOT, "mvtopicmodel_amd", "csrc"), "-o", str(lib), str(src)])
    return C.CDLL(str(lib))


def resolve(shim, request):
    q, out = (C.c_int * 9)(*request), (C.c_int * 7)()
    return tuple(out) if shim.flavour_resolve(q, out) else None


def compiled_keys(shim):
    keys = []
    for i in range(shim.flavour_count()):
        out = (C.c_int * 7)()
        shim.flavour_key(i, out)
        keys.append(tuple(out))
    return keys


def recorded():
    """request -> key or None, the table's wildcards written out; every request of DOMAIN exactly once"""
    want = {}
    for line in open(TABLE):
        if line.startswith("#") or not line.strip():
            continue
        pattern, outcome = line.split(":")
        fields = pattern.split()
        assert len(fields) == len(DOMAIN), line
        key = None if outcome.strip() == "-" else tuple(int(x) for x in outcome.split())
        assert key is None or len(key) == 7, line
        for request in itertools.product(*[dom if f == "*" else (int(f),) for f, dom in zip(fields, DOMAIN)]):
            assert request not in want, f"{request} is recorded twice"
            want[request] = key
    assert set(want) == set(itertools.product(*DOMAIN))
    return want


def test_every_request_resolves_to_what_the_two_ladders_chose(shim):
    want = recorded()
    assert len(want) == 5 * 5 * 3 * 2 ** 6
    wrong = [(request, resolve(shim, request), key) for request, key in want.items() if resolve(shim, request) != key]
    assert not wrong, f"{len(wrong)} requests differ, the first (request, got, recorded): {wrong[0]}"


def test_the_rule_names_exactly_the_kernels_that_are_compiled(shim):
    keys = compiled_keys(shim)
    assert len(keys) == 56 and len(set(keys)) == 56
    # beyond the recorded K: every K at which a threshold could sit, and none
    ks = (0, 1, 255, 256, 257, 511, 512, 513, 1023, 1024, 1025, 2048, 1 << 20)
    got = {resolve(shim, r) for r in itertools.product(DOMAIN[0], ks, *DOMAIN[2:])}
    got.discard(None)
    assert got == set(keys) - NEVER_RESOLVED
    assert NEVER_RESOLVED <= set(keys)                              # (still compiled: this list is not where a kernel is dropped)
    # the 12-bit flavour: the variants up to MVHDP_SLIM_MAX_ROUNDS have it, all of them, and no wider one
    assert {k[0] for k in keys if k[3] == 2} == {r for r in DOMAIN[0] if r <= shim.slim_max_rounds()}
    # rounds that are no variant's, and 3, which the 4-round variant takes
    assert all(resolve(shim, (r, 400, 0, 1, 1, 0, 0, 0, 0)) is None for r in (0, 5, 32, -1))
    assert resolve(shim, (3, 400, 0, 1, 1, 0, 0, 0, 0)) == (4, 0, 1, 1, 0, 0, 0)
