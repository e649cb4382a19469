"""Dispatch arithmetic of the slab-mode 3x3x3 launches (csrc/conv3.hip: slab_pick), through the query unetr_conv3_slab_dispatch:
no launch, no GPU.  For the eight launches of decoder5 (12^3) and decoder4 (24^3) at batch 2, and for the shapes of
test_conv_lowres_gpu.py, the grid never exceeds the workgroups the chip holds of the chosen kernel variant, the tiles are dealt so
that two workgroups differ by at most one, and a workgroup that walks more than one tile sits in a grid that is a multiple of the 8
XCDs (the walk is then in batch order, which the fused statistics need)."""
import ctypes

import pytest

CUS = 256
LDS_PER_CU = 160 * 1024
WINDOW_BYTES = 6 * 6 * 18 * 64
MAX_ROWS = 1024          # UNETR_CONV3_MAX_ROWS

# (B, D, H, W, contraction channels, produced channels, FUSE) -> (ntb, wl, grid.x, grid.y): bf16, the rule's own choice
REAL = {
    (2, 12, 12, 12, 256, 128, 2): (1, 1, 18, 8),
    (2, 12, 12, 12, 128, 128, 1): (1, 1, 18, 8),
    (2, 12, 12, 12, 128, 128, 5): (1, 1, 18, 8),
    (2, 12, 12, 12, 128, 256, 4): (2, 1, 18, 8),
    (2, 24, 24, 24, 128, 64, 2): (4, 1, 144, 1),
    (2, 24, 24, 24, 64, 64, 1): (4, 1, 144, 1),
    (2, 24, 24, 24, 64, 64, 5): (4, 1, 144, 1),
    (2, 24, 24, 24, 64, 128, 4): (2, 1, 48, 4),
}
TEST_SHAPES = [(1, 5, 12, 12, 64, 32), (1, 4, 24, 24, 32, 32), (1, 6, 10, 20, 96, 64), (1, 4, 8, 8, 32, 16), (2, 4, 12, 40, 64, 64),
               (1, 5, 12, 12, 32, 64), (1, 6, 10, 20, 64, 96), (2, 4, 12, 40, 64, 64)]
CFGS = [None, "1,2", "1,1", "2,2", "2,1", "4,1", "4,0"]


def _query(pkg, shape, prec, fuse):
    o = (ctypes.c_int * 6)()
    rc = pkg._capi.load().unetr_conv3_slab_dispatch(*shape, prec, fuse, o)
    return rc, tuple(o)


def _tiles(shape):
    B, D, H, W = shape[:4]
    return B * -(-W // 16) * -(-H // 4) * -(-D // 4)


def _check(shape, got, what):
    ntb, wl, gx, gy, resident, lds = got
    tiles = _tiles(shape)
    assert ntb in (1, 2, 4) and (shape[5] // 16) % ntb == 0 and gy == shape[5] // 16 // ntb, what
    assert lds == WINDOW_BYTES + wl * 27 * ntb * 1024 and lds <= LDS_PER_CU, what
    assert resident in (CUS, 2 * CUS) and resident <= CUS * (LDS_PER_CU // lds), what
    assert 1 <= gx <= min(tiles, MAX_ROWS) and gx * gy <= resident, f"{what}: grid {gx} x {gy} on {resident} resident workgroups"
    walks = [len(range(b, tiles, gx)) for b in range(gx)]
    assert max(walks) - min(walks) <= 1 and min(walks) >= 1, what
    assert gx == tiles or gx % 8 == 0, f"{what}: a walking grid of {gx} workgroups is not a multiple of the 8 XCDs"


@pytest.mark.parametrize("shape,want", REAL.items(), ids=lambda v: "x".join(map(str, v)) if len(v) == 7 else None)
def test_decoder5_and_decoder4_launches(pkg, monkeypatch, shape, want):
    monkeypatch.delenv("UNETR_CONV3_SLAB_CFG", raising=False)
    monkeypatch.delenv("UNETR_TEST_MAX_WG", raising=False)
    rc, got = _query(pkg, shape[:6], 1, shape[6])
    assert rc == 0
    _check(shape, got, str(shape))
    assert got[:4] == want, f"{shape}: dispatched as {got[:4]}, the measured table of slab_pick says {want}"
    # one tile per workgroup wherever statistics rows are written: the rows are the previous dispatch's rows, bit for bit
    if shape[6] != 4:
        assert got[2] == _tiles(shape)


@pytest.mark.parametrize("cfg", CFGS, ids=str)
@pytest.mark.parametrize("max_wg", [0, 8, 20])
def test_every_form_on_the_test_shapes(pkg, monkeypatch, cfg, max_wg):
    monkeypatch.delenv("UNETR_CONV3_SLAB_CFG", raising=False)
    monkeypatch.delenv("UNETR_TEST_MAX_WG", raising=False)
    if cfg:
        monkeypatch.setenv("UNETR_CONV3_SLAB_CFG", cfg)
    if max_wg:
        monkeypatch.setenv("UNETR_TEST_MAX_WG", str(max_wg))
    for shape in TEST_SHAPES + [s[:6] for s in REAL]:
        for prec in (0, 1, 2):
            for fuse in range(6):
                rc, got = _query(pkg, shape, prec, fuse)
                assert rc == 0, (shape, prec, fuse)
                _check(shape, got, f"{shape} prec {prec} fuse {fuse} cfg {cfg} max_wg {max_wg}")
                if max_wg:
                    assert got[2] <= max(8, max_wg // 8 * 8) or got[2] == _tiles(shape)


def test_levels_with_many_tiles_keep_their_grids(pkg, monkeypatch):
    """48^3 and 96^3 at batch 2 (864 / 6912 tiles): the generic rule, as before"""
    monkeypatch.delenv("UNETR_CONV3_SLAB_CFG", raising=False)
    monkeypatch.delenv("UNETR_TEST_MAX_WG", raising=False)
    assert _query(pkg, (2, 48, 48, 48, 64, 32), 1, 2)[1][:4] == (2, 2, 256, 1)
    assert _query(pkg, (2, 96, 96, 96, 32, 16), 1, 3)[1][:4] == (1, 1, 512, 1)
    monkeypatch.setenv("UNETR_CONV3_SLAB_CFG", "old")
    assert _query(pkg, (2, 24, 24, 24, 128, 64), 1, 2)[1][:4] == (1, 2, 144, 4)
    assert _query(pkg, (2, 12, 12, 12, 128, 256), 1, 4)[1][:4] == (1, 2, 18, 16)


def test_shapes_outside_slab_mode_are_declined(pkg):
    assert _query(pkg, (2, 96, 96, 96, 16, 16), 1, 1)[0] == 3          # pair mode (<= 16 contraction channels in bf16)
    assert _query(pkg, (1, 8, 8, 8, 32, 24), 1, 0)[0] == 3             # Cout % 16
    assert _query(pkg, (1, 8, 8, 8, 32, 16), 1, 6)[0] == 1
