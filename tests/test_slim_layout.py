"""The 12-bit image of n_wk (mvtopicmodel_amd/csrc/mvhdp_slim.h): the layout functions the tree build writes a row with and the
sweep kernels gather a cell with, compiled here with the host compiler -- one definition for all three.  A row is 128-byte aligned,
line j holds cells 85 j .. 85 j + 84 at 12 bits each, no cell crosses a line, bytes no cell uses stay zero."""
import ctypes as C
import os
import shutil
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KS = [1, 84, 85, 86, 170, 171, 255, 256, 400, 1000, 2048]

SHIM = r"""
#include "mvhdp_slim.h"
extern "C" {
unsigned long long slim_row_bytes(int K) { return mvhdp_slim_row_bytes(K); }
unsigned int slim_byte(int k) { return mvhdp_slim_byte(k); }
unsigned int slim_shift(int k) { return mvhdp_slim_shift(k); }
unsigned int slim_get(const unsigned char* row, int k) { return mvhdp_slim_get(row, k); }
void slim_put(unsigned char* row, int k, unsigned int v) { mvhdp_slim_put(row, k, v); }
int slim_pays(int K, int max_types, int level) { return mvhdp_slim_pays(K, max_types, level); }
}
"""


@pytest.fixture(scope="module")
def shim(tmp_path_factory):
    cxx = shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
    if cxx is None:
        pytest.fail("no host C++ compiler: the layout header cannot be checked")
    d = tmp_path_factory.mktemp("slim")
    src, lib = d / "slim_shim.cpp", d / "libslim_shim.so"
    src.write_text(SHIM)
    subprocess.check_call([cxx, "-std=c++17", "-O1", "-Wall", "-Werror", "-shared", "-fPIC",
                           "-I", os.path.join(ROOT, "mvtopicmodel_amd", "csrc"), "-o", str(lib), str(src)])
    L = C.CDLL(str(lib))
    L.slim_row_bytes.restype = C.c_ulonglong
    for f in (L.slim_byte, L.slim_shift, L.slim_get, L.slim_pays):
        f.restype = C.c_uint
    L.slim_get.argtypes = [C.c_void_p, C.c_int]
    L.slim_put.argtypes = [C.c_void_p, C.c_int, C.c_uint]
    return L


@pytest.mark.parametrize("K", KS)
def test_every_cell_unpacks_to_itself_and_stays_inside_its_line(shim, K):
    rng = np.random.RandomState(K)
    stride = shim.slim_row_bytes(K)
    lines = (K + 84) // 85
    assert stride == 128 * lines
    nrows = 5
    vals = rng.randint(0, 4096, size=(nrows, K)).astype(np.uint32)
    vals[0, :] = 4095                                   # every bit of every cell
    vals[1, :] = 0
    vals[2, ::2] = 4095; vals[2, 1::2] = 0              # neighbours that must not leak into each other
    vals[3, ::2] = 0; vals[3, 1::2] = 4095
    buf = np.zeros(nrows * stride + 2, dtype=np.uint8)
    used = np.zeros(stride, dtype=bool)
    for k in range(K):
        b, sh = shim.slim_byte(k), shim.slim_shift(k)
        j, i = divmod(k, 85)
        assert b == 128 * j + ((3 * i) >> 1) and sh == 4 * (i & 1)
        assert b // 128 == (b + 1) // 128 == j, f"cell {k} crosses a line"
        assert b + 1 < stride
        used[b] = used[b + 1] = True
    for r in range(nrows):
        row = buf[r * stride:].ctypes.data
        for k in range(K):
            shim.slim_put(row, k, int(vals[r, k]))
    for r in range(nrows):
        row = buf[r * stride:].ctypes.data
        got = np.array([shim.slim_get(row, k) for k in range(K)], dtype=np.uint32)
        assert np.array_equal(got, vals[r]), f"row {r}"
        # the same through the definition of the issue: the 16 bits at the byte offset, little-endian, shifted and masked
        raw = buf[r * stride:(r + 1) * stride]
        byte = np.array([shim.slim_byte(k) for k in range(K)]); shift = np.array([shim.slim_shift(k) for k in range(K)])
        u16 = raw[byte].astype(np.uint32) | (raw[byte + 1].astype(np.uint32) << 8)
        assert np.array_equal((u16 >> shift) & 0xfff, vals[r])
    assert not buf[nrows * stride:].any()                # nothing written behind the last row
    tail = buf[:nrows * stride].reshape(nrows, stride)[:, ~used]
    assert not tail.any(), "bytes no cell uses are zero"
    # the last 4 bits of a full line belong to no cell either
    full = buf[:nrows * stride].reshape(nrows, stride)[0]
    for j in range(K // 85):
        assert full[128 * j + 127] >> 4 == 0


def test_lines_of_a_row_at_the_benchmark_sizes(shim):
    assert shim.slim_row_bytes(400) == 5 * 128 and shim.slim_row_bytes(1000) == 12 * 128 and shim.slim_row_bytes(200) == 3 * 128


def test_where_the_image_is_kept(shim):
    """Fewer lines than a row of the 16-bit mirror spans at the least, rows long enough for the lines to matter, and type ids that
    leave bit 28 free: the library accepts views of up to 2^29 - 1 types, and a handle with a view of 2^28 or more keeps the mirror."""
    V = 50_000
    assert [shim.slim_pays(K, V, 1) for K in (100, 200, 400, 1000)] == [0, 0, 1, 1]
    assert [shim.slim_pays(K, V, 2) for K in (100, 200, 400, 1000)] == [0, 1, 1, 1]      # K = 100: 2 lines either way
    assert [shim.slim_pays(K, V, 0) for K in (100, 200, 400, 1000)] == [0, 0, 0, 0]
    assert shim.slim_pays(256, V, 2) == 0 and shim.slim_pays(257, V, 1) == 1             # 4 lines against 4, then against 5
    assert shim.slim_pays(400, (1 << 28) - 1, 1) == 1
    assert shim.slim_pays(400, 1 << 28, 1) == 0 and shim.slim_pays(400, (1 << 29) - 1, 2) == 0
