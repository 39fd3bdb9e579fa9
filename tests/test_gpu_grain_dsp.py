"""GPU parity of the per-call film grain table
(Dav1dFilmGrainDSPContext_{8bpc,16bpc}, src/filmgrain.h:46-80), called
through ctypes function pointers the way dav1d_prep_grain and
dav1d_apply_grain_row call it (src/fg_apply_tmpl.c:100-223), against the
oracle's whole-picture dav1d_apply_grain: its grain LUTs for
generate_grain_*, its pictures for fgy_32x32xn / fguv_32x32xn.  Bit-exact
bar; every buffer is sentinel-filled so a write outside the reference's
extent shows."""
import ctypes

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

BITDEPTHS = [(8, 255), (16, 1023), (16, 4095)]


def _table(pkg, bpc, hook="dav1d_film_grain_dsp_init", t=None):
    t = pkg.abi.FilmGrainDSPContext() if t is None else t
    getattr(pkg.abi.load_lib(), f"{hook}_{bpc}bpc")(ctypes.byref(t))
    return t


@pytest.mark.parametrize("bpc,bdmax", BITDEPTHS)
@pytest.mark.parametrize("layout", [1, 2, 3])
@pytest.mark.parametrize("lag", [0, 1, 2, 3])
def test_generate_grain(pkg, oracle, bpc, bdmax, layout, lag):
    """lag 1 runs without luma points: generate_grain_uv then has no luma
    term and does not read buf_y."""
    import dav1d_mirror_amd.grain as grain
    c = grain.make_grain_case(seed=1000 + 100 * layout + 10 * lag + bpc + bdmax, width=64, height=32, bpc=bpc,
                              bitdepth_max=bdmax, layout=layout, lag=lag, num_y=0 if lag == 1 else 5, csfl=False,
                              num_uv=(4, 6))
    _, g, _ = oracle.apply_grain(c)
    GY, GUV, _, _ = pkg.abi.film_grain_fn_types(bpc)
    hbd = () if bpc == 8 else (bdmax,)
    edt, S = (np.int8, 0x55) if bpc == 8 else (np.int16, 0x5555)
    t = _table(pkg, bpc)
    buf_y = np.full((74, 82), S, edt)
    GY(t.generate_grain_y)(buf_y.ctypes.data, ctypes.byref(c.data), *hbd)
    assert np.array_equal(buf_y[:73], g[0]), "generate_grain_y"
    assert (buf_y[73] == S).all(), "row 73 written"
    ch, cw = (38 if layout == 1 else 73), (44 if layout != 3 else 82)
    for uv in range(2):
        buf = np.full((74, 82), S, edt)
        GUV(t.generate_grain_uv[layout - 1])(buf.ctypes.data, buf_y.ctypes.data, ctypes.byref(c.data), uv, *hbd)
        assert np.array_equal(buf[:ch, :cw], g[1 + uv][:ch, :cw]), f"generate_grain_uv {uv}"
        assert (buf[ch:] == S).all() and (buf[:, cw:] == S).all(), f"generate_grain_uv {uv} wrote outside its extent"


def _apply_rows(pkg, t, c, g, sc):
    """dav1d_apply_grain_row for every strip (fg_apply_tmpl.c:161-223) on
    pictures of stride 96 with the oracle's LUTs; returns the output
    pictures (sentinel-filled before) and the sentinel."""
    bpc, d, layout = c.bpc, c.data, c.layout
    _, _, FGY, FGUV = pkg.abi.film_grain_fn_types(bpc)
    hbd = () if bpc == 8 else (c.bitdepth_max,)
    pdt, edt, S, SC = (np.uint8, np.int8, 0xA5, 256) if bpc == 8 else (np.uint16, np.int16, 0xA5A5, 4096)
    stride, bpp = 96, np.dtype(pdt).itemsize
    W, H = c.plane_wh[0]
    ss_x, ss_y = int(layout != 3), int(layout == 1)
    ins, outs = [], []
    for p, (w, h) in enumerate(c.plane_wh):
        a = np.zeros((h, stride), pdt)
        a[:, :w] = c.planes[p]
        ins.append(a)
        outs.append(np.full((h, stride), S, pdt))
    if W & ss_x:                                       # extend padding pixels (:195-202)
        ins[0][:, W] = ins[0][:, W - 1]
    lut = np.zeros((3, 74, 82), edt)
    lut[:, :73] = g
    scaling = np.ascontiguousarray(sc[:, :SC])
    cpw = (W + ss_x) >> ss_x
    addr = lambda a, y: a.ctypes.data + y * stride * bpp  # noqa: E731
    for row in range((H + 31) // 32):
        if d.num_y_points:
            bh = min(H - row * 32, 32)
            FGY(t.fgy_32x32xn)(addr(outs[0], row * 32), addr(ins[0], row * 32), stride * bpp, ctypes.byref(d), W,
                               scaling[0].ctypes.data, lut[0].ctypes.data, bh, row, *hbd)
        if not (d.num_uv_points[0] or d.num_uv_points[1] or d.chroma_scaling_from_luma):
            continue
        bh = (min(H - row * 32, 32) + ss_y) >> ss_y
        uv_row = (row * 32) >> ss_y
        for pl in range(2):
            if not (d.chroma_scaling_from_luma or d.num_uv_points[pl]):
                continue
            s = scaling[0] if d.chroma_scaling_from_luma else scaling[1 + pl]
            FGUV(t.fguv_32x32xn[layout - 1])(addr(outs[1 + pl], uv_row), addr(ins[1 + pl], uv_row), stride * bpp,
                                             ctypes.byref(d), cpw, s.ctypes.data, lut[1 + pl].ctypes.data, bh, row,
                                             addr(ins[0], row * 32), stride * bpp, pl, c.is_id, *hbd)
    return outs, S


@pytest.mark.parametrize("bpc,bdmax", BITDEPTHS)
@pytest.mark.parametrize("layout", [1, 2, 3])
@pytest.mark.parametrize("w,h", [(70, 66), (71, 34)])
@pytest.mark.parametrize("overlap", [False, True])
@pytest.mark.parametrize("csfl", [False, True])
def test_fgy_fguv_strips(pkg, oracle, bpc, bdmax, layout, w, h, overlap, csfl):
    import dav1d_mirror_amd.grain as grain
    c = grain.make_grain_case(seed=2000 + 7 * layout + bdmax + w + 2 * overlap + csfl, width=w, height=h, bpc=bpc,
                              bitdepth_max=bdmax, layout=layout, num_y=6, num_uv=(4, 5), csfl=csfl, overlap=overlap)
    want, g, sc = oracle.apply_grain(c)
    outs, S = _apply_rows(pkg, _table(pkg, bpc), c, g, sc)
    for p, (pw, ph) in enumerate(c.plane_wh):
        bad = np.argwhere(outs[p][:, :pw] != want[p])
        assert len(bad) == 0, f"plane {p}: {len(bad)} pixels differ, first {bad[:5].tolist()}"
        assert (outs[p][:, pw:] == S).all(), f"plane {p}: columns past pw written"


@pytest.mark.parametrize("bpc,bdmax", [(8, 255), (16, 1023)])
def test_gpu_hook_does_not_run_the_fallback(pkg, oracle, bpc, bdmax):
    """The _gpu_ hook over a caller's table keeps the caller's entries for
    failures only: without one they are never called."""
    import dav1d_mirror_amd.grain as grain
    c = grain.make_grain_case(seed=31 + bpc, width=70, height=34, bpc=bpc, bitdepth_max=bdmax, layout=1, num_y=6,
                              num_uv=(4, 5), csfl=False, overlap=True)
    want, g, sc = oracle.apply_grain(c)
    GY, GUV, FGY, FGUV = pkg.abi.film_grain_fn_types(bpc)
    calls = []
    cbs = [GY(lambda *a: calls.append("gy")), GUV(lambda *a: calls.append("guv")),
           FGY(lambda *a: calls.append("fgy")), FGUV(lambda *a: calls.append("fguv"))]
    addr = [ctypes.cast(cb, ctypes.c_void_p).value for cb in cbs]
    t = pkg.abi.FilmGrainDSPContext()
    t.generate_grain_y, t.fgy_32x32xn = addr[0], addr[2]
    for i in range(3):
        t.generate_grain_uv[i], t.fguv_32x32xn[i] = addr[1], addr[3]
    _table(pkg, bpc, "dav1d_film_grain_dsp_init_gpu", t)
    assert t.fgy_32x32xn != addr[2] and t.fguv_32x32xn[0] != addr[3] and t.generate_grain_y != addr[0]
    outs, _ = _apply_rows(pkg, t, c, g, sc)
    buf = np.zeros((74, 82), np.int8 if bpc == 8 else np.int16)
    GY(t.generate_grain_y)(buf.ctypes.data, ctypes.byref(c.data), *(() if bpc == 8 else (bdmax,)))
    assert calls == []
    assert pkg.abi.load_lib().dav1d_gpu_get_error() == 0
    assert np.array_equal(buf[:73], g[0])
    for p, (pw, ph) in enumerate(c.plane_wh):
        assert np.array_equal(outs[p][:, :pw], want[p]), p
