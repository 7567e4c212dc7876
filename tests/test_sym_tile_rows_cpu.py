"""rbpf_filter_workspace_bytes (no device needed) at the block-lower tile-row counts 6, 10, 12 and 14: storage = 2 reports the
lower block triangle plus the step kernel's column-strip workspace, not the full square."""
import ctypes as C
import importlib

import pytest

import cases

TILE = 64 * 64


def strip_doubles(ch, de=3):
    """Column strips of row pairs 1 .. ch / 2 - 1 (rows {rp, ch - 1 - rp}; strip of rp: columns [0, 64 (ch - 1 - rp)))."""
    return sum(de * 64 * (ch - 1 - rp) for rp in range(1, ch // 2))


@pytest.mark.parametrize("m", [384, 640, 768, 896])
def test_block_lower_workspace_at_the_new_tile_row_counts(rbpf, m):
    ffi = importlib.import_module(rbpf.__name__ + "._ffi")
    host = importlib.import_module(rbpf.__name__ + ".host")
    lib = rbpf.load_library()
    c = cases.mag_case(16, 3, m, seed=1)
    mdl, x0, P0, R = cases.device_model(rbpf, c)
    prob = host._Problem(mdl, c["odometry"], c["y"], c["x0_nonLin"], x0, P0, c["Q"], R, c["N_P"], c["dt"])
    mdesc = mdl.descriptor()
    need = {}
    for storage in (0, 2):
        nbytes = C.c_size_t(0)
        opt = ffi.rbpf_options(keep_history=1, storage=storage, lazy_depth=3)
        assert lib.rbpf_filter_workspace_bytes(C.byref(mdesc), C.byref(prob.c), C.byref(opt), C.byref(nbytes)) == rbpf.RBPF_OK
        need[storage] = nbytes.value
    n, N = m + 3, 16
    mc = (n // 128) * 128
    ch = mc // 64
    assert ch in (6, 10, 12, 14)
    assert need[2] < need[0]
    saved = (2 * N + 1) * (n * mc - ch * (ch + 1) // 2 * TILE) * 8    # two banks and the packed P0: core rows of the square vs tiles
    strips = N * strip_doubles(ch) * 8
    assert abs((need[0] - need[2]) - (saved - strips)) <= 0.02 * saved, (need[0] - need[2], saved, strips)
