"""The channel-split wave mapping of the small-tile conv kernel - what can be checked without a GPU: bpx_debug_set_conv_wn and
bpx_conv3d_wn_supported are declared, exported and bound; the statistics-tile and workspace queries answer the same whatever WN is set; the
instance query admits WN <= NS on the 4x4x8 16-bit shapes only."""
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture()
def L():
    from biapy_amd import _lib

    yield _lib
    _lib.lib.bpx_debug_set_conv_wn(-1)


def test_hook_and_query_are_declared_exported_and_bound(L):
    header = open(os.path.join(ROOT, "include", "biapy_amd.h")).read()
    assert re.search(r"^int bpx_debug_set_conv_wn\(int wn\);", header, re.M)
    assert re.search(r"^int bpx_conv3d_wn_supported\(int dtype, int D, int H, int W, int Cout, int wn\);", header, re.M)
    i = L.C.c_int
    assert L._SIGS["bpx_debug_set_conv_wn"] == ([i], i)
    assert L._SIGS["bpx_conv3d_wn_supported"] == ([i] * 6, i)
    assert {"bpx_debug_set_conv_wn", "bpx_conv3d_wn_supported"} <= set(L.EXPORTS)
    for wn in (-1, 0, 1, 2, 4):
        assert L.lib.bpx_debug_set_conv_wn(wn) == 0


def test_queries_do_not_depend_on_wn(L):
    lib = L.lib
    shapes = [(2, 8, 8, 8, 64, 32), (2, 6, 10, 12, 48, 64), (1, 16, 16, 16, 384, 128), (2, 4, 4, 4, 256, 256), (1, 32, 32, 32, 64, 64)]

    def answers():
        out = []
        for N, D, H, W, Cin, Cout in shapes:
            for dt in (L.F32, L.BF16, L.F16):
                out.append(lib.bpx_conv3d_stats_tiles(dt, N, D, H, W, Cout))
            out.append(lib.bpx_conv3d_wgrad_workspace(N, D, H, W, Cin, Cout, 3))
            out.append(lib.bpx_conv3d_bwd_fused_stats_tiles(N, D, H, W, Cout, Cin))
            out.append(lib.bpx_conv3d_bwd_fused_workspace(N, D, H, W, Cout, Cin))
        return out

    lib.bpx_debug_set_conv_wn(1)
    want = answers()
    for wn in (-1, 0, 2, 4):
        lib.bpx_debug_set_conv_wn(wn)
        assert answers() == want, wn


def test_instance_query(L):
    q = L.lib.bpx_conv3d_wn_supported
    for dt in (L.BF16, L.F16, L.MIX16):
        assert q(dt, 16, 16, 16, 128, 2) == 1 and q(dt, 16, 16, 16, 128, 4) == 1      # NS 4
        assert q(dt, 8, 8, 8, 256, 2) == 1 and q(dt, 8, 8, 8, 256, 4) == 0            # NS 2 at <= 8^3
        assert q(dt, 6, 10, 12, 32, 2) == 1 and q(dt, 6, 10, 12, 32, 4) == 0          # NS 2
        assert q(dt, 6, 10, 12, 48, 2) == 0 and q(dt, 6, 10, 12, 16, 2) == 0          # NS 3, NS 1
        assert q(dt, 32, 32, 32, 64, 2) == 0                                          # 4x4x16 tiles
        assert q(dt, 32, 32, 32, 64, 1) == 1 and q(dt, 8, 8, 8, 64, 3) == 0
    assert L.lib.bpx_conv3d_wn_supported(L.F32, 8, 8, 8, 64, 2) == 0 and L.lib.bpx_conv3d_wn_supported(L.F32, 8, 8, 8, 64, 1) == 1
