"""`ort_mtf_map_f64`: sagittal and tangential OTF / MTF of OPD maps on the device, against the definition in include/ort.h
evaluated by numpy in complex128, shear by shear as `tests/test_gpu_mtf.py` does it: the shifted products of the pupil field,
the mirrored map built explicitly by concatenation, the conjugate for a negative step, divided by the mask sum.  No Gram
matrix and nothing shared with the kernel.  Bound 1e-11 absolute on values of modulus <= 1, the bound of `ort_mtf_f64` and
`ort_psf_map_f64`: sums of at most 2048^2 unit-modulus terms divided by N."""
import numpy as np
import pytest

import opticalraytracing_jl_amd as ort
from tests import common as cm

pytestmark = pytest.mark.gpu
TOL = 1e-11


def reference_otf(opd, step, nshear, mirror):
    """(H [nb][2][nshear] complex, N [nb]); samples at or past an axis's width are 0, and NaN where N = 0."""
    H, cnt = np.zeros((len(opd), 2, nshear), dtype=np.complex128), []
    for b, (W, (dpy, dpx)) in enumerate(zip(opd, step)):
        if mirror:
            W = np.concatenate([W[:, :0:-1], W], axis=1)
        mask = ~np.isnan(W)
        P = np.where(mask, np.exp(2j * np.pi * np.nan_to_num(W)), 0.0)
        for axis, (Q, dp) in enumerate(((P, dpx), (P.T, dpy))):      # the shear runs along Q's second index
            L = Q.shape[1]
            for d in range(min(L, nshear)):
                h = (Q[:, d:] * np.conj(Q[:, :L - d])).sum()
                H[b, axis, d] = np.conj(h) if dp < 0 else h
        with np.errstate(invalid="ignore"):
            H[b] /= np.float64(mask.sum())
        cnt.append(mask.sum())
    return H, np.array(cnt)


def wavefront_maps(rng, nb, ny, nx, mirror, rms):
    """nb maps in the style of test_gpu_psf_map's: smooth (even in x under mirror) plus 5 % noise, scaled to `rms` waves, on a
    disc (even b) or on the lens-shaped intersection of two discs (odd b); steps per bundle, dpy negative on odd bundles."""
    u = np.arange(nx) / nx if mirror else (2.0 * np.arange(nx) + 1.0 - nx) / nx
    X, Y = np.meshgrid(u, (2.0 * np.arange(ny) + 1.0 - ny) / ny)
    c = rng.normal(size=(nb, 4, 1, 1))
    W = c[:, 0] * (X * X + Y * Y) + c[:, 1] * (X * X - Y * Y) + c[:, 2] * (3 * (X * X + Y * Y) - 2) * Y + c[:, 3] * X * (1 - mirror)
    W += 0.05 * W.std(axis=(1, 2), keepdims=True) * rng.normal(size=W.shape)
    lens = (np.arange(nb) % 2 == 1)[:, None, None]
    W[~((X * X + Y * Y <= 1.0) & (~lens | (X * X + (Y - 0.6) ** 2 <= 1.0)))] = np.nan
    W *= np.reshape(rms, (-1, 1, 1)) / np.nanstd(W, axis=(1, 2), keepdims=True)
    step = rng.uniform(0.8, 1.2, size=(nb, 2)) * [2.0 / ny, (1.0 if mirror else 2.0) / nx]
    step[1::2, 0] *= -1.0
    return W, step


def deviation(mtf, otf, want):
    return max(np.abs(otf - want).max(), np.abs(mtf - np.abs(want)).max())


@pytest.mark.parametrize("ny,nx,nshear,mirror", ((16, 16, 16, False), (22, 11, 21, True), (80, 48, 80, False), (80, 48, 20, False),
                                                 (33, 272, 272, False), (64, 32, 64, True)))
def test_mtf_map_matches_direct_sum(hip_engine, ny, nx, nshear, mirror):
    """One block (no r < c tile); ragged both ways plus mirror; spans and fold, axis 0 only 48 wide so its samples 48..79 are
    exactly 0; fewer diagonals than the width has; 17 block diagonals in two groups with 33 lines and axis 1 only 33 wide;
    api.opd's default shape.  Bundle 2 is an all-NaN map."""
    import torch
    rng = np.random.default_rng(43000 + ny + nx + nshear)
    opd, step = wavefront_maps(rng, 3, ny, nx, mirror, [0.1, 1.0, 0.5])
    opd[2] = np.nan
    want, n = reference_otf(opd, step, nshear, mirror)
    mtf, otf, count = hip_engine.mtf_map(opd, step, nshear, mirror_x=mirror, want_otf=True)
    dev = deviation(mtf[:2], otf[:2], want[:2])
    print(f"mtf_map ({ny}, {nx}, {nshear}, {mirror}): worst deviation {dev:.3e}, H(0) - 1 = {abs(otf[0, 0, 0] - 1):.1e}, N {count}")
    cm.report(f"mtf_map {ny} x {nx} nshear {nshear} mirror {mirror}: worst deviation from the direct sum {dev:.2e} (bound {TOL:g})")
    assert dev <= TOL
    assert np.array_equal(mtf[:2], np.hypot(otf[:2].real, otf[:2].imag))
    assert np.isnan(mtf[2]).all() and np.isnan(otf[2].real).all() and np.isnan(otf[2].imag).all() and count[2] == 0
    assert np.array_equal(count, n)
    for axis, width in enumerate((2 * nx - 1 if mirror else nx, ny)):  # past the width: exactly +0
        tail = np.stack((otf[:2, axis, width:].real, otf[:2, axis, width:].imag, mtf[:2, axis, width:]))
        assert np.all(tail == 0.0) and not np.signbit(tail).any()
    only, none, cnt = hip_engine.mtf_map(opd, step, nshear, mirror_x=mirror)
    assert none is None and np.array_equal(only, mtf, equal_nan=True) and np.array_equal(cnt, count)
    d = [torch.from_numpy(a).to(torch.device("cuda:0")) for a in (opd, step)]
    torch.cuda.synchronize()
    runs = [hip_engine.mtf_map(d[0], d[1], nshear, mirror_x=mirror, want_otf=True) for _ in range(2)]
    hip_engine.ctx.synchronize()
    for dm, do, dc in runs:                                           # device pointers == host pointers, and run to run
        assert np.array_equal(dm.cpu().numpy(), mtf, equal_nan=True) and np.array_equal(dc.cpu().numpy(), count)
        assert np.array_equal(torch.view_as_real(do).cpu().numpy(), np.stack((otf.real, otf.imag), axis=-1), equal_nan=True)


@pytest.mark.parametrize("nb,ny,nx,nshear,mirror", ((1200, 20, 24, 24, False), (1100, 22, 11, 21, True)))
def test_many_bundles_route(hip_engine, nb, ny, nx, nshear, mirror):
    """More units than four workgroups per compute unit: one workgroup per (bundle, axis), N divided out at the end, no
    workspace.  Every bundle has its own map and step, so an index mix-up between bundles fails."""
    rng = np.random.default_rng(43415 + nshear)
    opd, step = wavefront_maps(rng, nb, ny, nx, mirror, rng.uniform(0.05, 1.0, size=nb))
    want, n = reference_otf(opd, step, nshear, mirror)
    mtf, otf, count = hip_engine.mtf_map(opd, step, nshear, mirror_x=mirror, want_otf=True)
    dev = deviation(mtf, otf, want)
    cm.report(f"mtf_map, {nb} bundles, mirror {mirror}: worst deviation from the direct sum {dev:.2e} (bound {TOL:g})")
    assert dev <= TOL and np.array_equal(count, n)
    assert np.array_equal(mtf, np.hypot(otf.real, otf.imag))


def test_conventions(hip_engine):
    """Normalisation, sign and shear direction, independently of the reference function: a flat map with a ragged mask; a tilt
    W = 2 a x with +dpx, and with the columns reversed and -dpx; a map sampled from a Zernike wavefront on ort_mtf_f64's own
    grid gives ort_mtf_f64's curves."""
    rng = np.random.default_rng(43999)
    # every row and every column of the mask is one run of random length about column 13 (unimodal half-widths): a ragged
    # outline whose overlap with its own shifted copy cannot grow with the shift, which scattered holes would not guarantee
    hl, hr = (np.concatenate([v[::2], v[1::2][::-1]]) for v in np.sort(rng.integers(1, 14, size=(2, 19)), axis=1))
    k = np.arange(27)
    flat = np.where((k >= 13 - hl[:, None]) & (k <= 13 + hr[:, None]), 0.0, np.nan)[None]
    mtf, otf, _ = hip_engine.mtf_map(flat, np.array([[0.07, -0.05]]), 27, want_otf=True)
    assert np.abs(otf[0, :, 0] - 1.0).max() <= 1e-12 and np.all(otf.imag == 0.0) and np.all(np.diff(mtf[0], axis=1) <= 0.0)
    a, npupil, dp = 0.375, 32, 2.0 / 32
    tilt, d = np.tile(2 * a * np.arange(npupil) * dp, (1, npupil, 1)), np.arange(npupil)
    for W, dpx in ((tilt, dp), (tilt[:, :, ::-1], -dp)):
        mtf, otf, _ = hip_engine.mtf_map(np.ascontiguousarray(W), np.array([[dp, dpx]]), npupil, want_otf=True)
        sel = mtf[0, 0] > 0.01
        assert sel.sum() > npupil // 2
        assert np.abs(np.angle(otf[0, 0] * np.exp(-2j * np.pi * 2 * a * d * dp)))[sel].max() <= 1e-11
    x = (2.0 * np.arange(npupil) + 1.0 - npupil) / npupil
    X, Y = np.meshgrid(x, x)
    r2, terms, coef = X * X + Y * Y, ort.zernike_terms(4), np.zeros((1, 14))
    W = np.zeros_like(X)
    for (n, m), c, Z in (((1, 1), 0.2, 2 * X), ((2, 0), -0.15, np.sqrt(3) * (2 * r2 - 1)), ((2, 2), 0.1, np.sqrt(6) * (X * X - Y * Y)),
                         ((3, 1), 0.12, np.sqrt(8) * (3 * r2 - 2) * X), ((4, 0), -0.08, np.sqrt(5) * (6 * r2 * r2 - 6 * r2 + 1))):
        coef[0, terms.index((n, m))] = c
        W += c * Z
    W[r2 > 1.0] = np.nan
    want_m, want_o = hip_engine.mtf(coef, 4, npupil, want_otf=True)
    mtf, otf, count = hip_engine.mtf_map(W[None], np.full((1, 2), dp), npupil, want_otf=True)
    assert deviation(mtf, otf, want_o) <= TOL and np.abs(mtf - want_m).max() <= TOL and count[0] == (r2 <= 1.0).sum()


def test_mtf_opd(hip_engine):
    """api.mtf_opd is opd() plus mtf_map on the half map with psf_opd's steps; the parabola on axis has W = 0."""
    system = ort.solve(cm.cooke(), cm.COOKE_A, cm.COOKE_H, engine=hip_engine)
    fs, ms, ft, mt = ort.mtf_opd(system, 0.7, engine=hip_engine)
    w = ort.opd(system, 0.7, engine=hip_engine)
    step = np.array([[(w.y[1] - w.y[0]) / w.x[-1], (w.x[1] - w.x[0]) / w.x[-1]]])
    ny, nx = w.opd.shape
    m = hip_engine.mtf_map(w.opd[None], step, max(ny, 2 * nx - 1), mirror_x=True)[0]
    assert np.array_equal(ms, m[0, 0]) and np.array_equal(mt, m[0, 1]) and len(fs) == max(ny, 2 * nx - 1)
    assert np.array_equal(fs, np.arange(len(fs)) * abs(step[0, 1])) and np.array_equal(ft, np.arange(len(ft)) * abs(step[0, 0]))
    parabola = ort.solve(ort.Layout(cm.parabola_M(), profile=ort.Aspheric), np.full(1, 30.0), 21.0, engine=hip_engine)
    wp = ort.opd(parabola, 0.0, k_rays=32, engine=hip_engine)
    stp = np.array([[(wp.y[1] - wp.y[0]) / wp.x[-1], (wp.x[1] - wp.x[0]) / wp.x[-1]]])
    zero = hip_engine.mtf_map(np.where(np.isnan(wp.opd), np.nan, 0.0)[None], stp, 32, mirror_x=True)[0]
    _, ps, _, pt = ort.mtf_opd(parabola, 0.0, k_rays=32, engine=hip_engine)
    assert np.abs(ps - zero[0, 0]).max() <= 1e-9 and np.abs(pt - zero[0, 1]).max() <= 1e-9
    fit = ort.zernike_fit(ort.full_trace(system, 0.0, engine=hip_engine), 10, engine=hip_engine)[0]
    ff, fsag, _ = ort.mtf(fit, 10, engine=hip_engine)
    f0, m0, _, _ = ort.mtf_opd(system, 0.0, engine=hip_engine)
    cm.report(f"mtf_opd, Cooke H = 0, sagittal MTF at 0.5 cycles per wavegrad unit: {np.interp(0.5, f0, m0):.4f} from the OPD map, "
              f"{np.interp(0.5, ff, fsag):.4f} from the degree-10 Zernike fit")


@pytest.mark.parametrize("kw", (dict(ny=0), dict(nx=2049), dict(nx=1025, flags=1 << 11), dict(nshear=0), dict(nshear=2049),
                                dict(opd=None), dict(step=None), dict(mtf=None)))
def test_bad_arguments(hip_engine, kw):
    z = np.zeros(4096)
    a = dict(ny=4, nx=4, nshear=16, opd=z.ctypes.data, step=z.ctypes.data, mtf=z.ctypes.data, flags=0)
    a.update(kw)
    rc = hip_engine.ctx.lib.ort_mtf_map_f64(hip_engine.ctx.h, 1, a["ny"], a["nx"], a["opd"], a["step"], a["nshear"], None, a["mtf"], None,
                                            a["flags"])
    assert rc == -1                                                   # ORT_EINVAL
