"""`ort_psf_map_f64`: diffraction PSF and Strehl ratio of OPD maps on the device, against the definition evaluated by numpy in
complex128 — `abs(Ey @ P @ Ex.T) ** 2 / N ** 2` with plain exponential tables, the mirrored map built explicitly by
concatenation.  Nothing shared with the kernel's factorised twiddles.  Bound 1e-11 absolute on values <= 1, the bound of
`ort_psf_f64`: both the plain and the factorised float64 form lie within 4e-17 of a long-double direct sum on these shapes."""
import numpy as np
import pytest

import opticalraytracing_jl_amd as ort
from tests import common as cm

pytestmark = pytest.mark.gpu
TOL, DXI = 1e-11, 0.125


def reference_psf(opd, step, nimg, centre, mirror):
    """(psf [nb][nimg][nimg], N [nb]) by the definition in include/ort.h, bundle by bundle; NaN where N = 0."""
    m, out, cnt = (np.arange(nimg) - nimg // 2) * DXI, [], []
    for W, (dpy, dpx), (xc, yc) in zip(opd, step, centre):
        y, x = np.arange(W.shape[0]) * dpy, np.arange(W.shape[1]) * dpx
        if mirror:
            W, x, xc = np.concatenate([W[:, :0:-1], W], axis=1), np.concatenate([-x[:0:-1], x]), 0.0
        mask = ~np.isnan(W)
        P = np.where(mask, np.exp(2j * np.pi * np.nan_to_num(W)), 0.0)
        Ex, Ey = np.exp(-2j * np.pi * np.outer(xc + m, x)), np.exp(-2j * np.pi * np.outer(yc + m, y))
        with np.errstate(invalid="ignore"):
            out.append(np.abs(Ey @ P @ Ex.T) ** 2 / np.float64(mask.sum()) ** 2)
        cnt.append(mask.sum())
    return np.array(out), np.array(cnt)


def wavefront_maps(rng, nb, ny, nx, mirror, rms):
    """nb maps: smooth (defocus, astigmatism, coma; even in x under mirror) plus 5 % noise, scaled to `rms` waves each, on a
    disc (even b) or on the lens-shaped intersection of two discs, a vignetted field (odd b); steps and centres per bundle."""
    u = np.arange(nx) / nx if mirror else (2.0 * np.arange(nx) + 1.0 - nx) / nx
    X, Y = np.meshgrid(u, (2.0 * np.arange(ny) + 1.0 - ny) / ny)
    c = rng.normal(size=(nb, 4, 1, 1))
    W = c[:, 0] * (X * X + Y * Y) + c[:, 1] * (X * X - Y * Y) + c[:, 2] * (3 * (X * X + Y * Y) - 2) * Y + c[:, 3] * X * (1 - mirror)
    W += 0.05 * W.std(axis=(1, 2), keepdims=True) * rng.normal(size=W.shape)
    lens = (np.arange(nb) % 2 == 1)[:, None, None]
    W[~((X * X + Y * Y <= 1.0) & (~lens | (X * X + (Y - 0.6) ** 2 <= 1.0)))] = np.nan
    W *= np.reshape(rms, (-1, 1, 1)) / np.nanstd(W, axis=(1, 2), keepdims=True)
    step = rng.uniform(0.8, 1.2, size=(nb, 2)) * [2.0 / ny, (1.0 if mirror else 2.0) / nx]
    step[1::2, 0] *= -1.0                                             # an axis that runs downward
    return W, step, rng.uniform(-0.5, 0.5, size=(nb, 2))


@pytest.mark.parametrize("ny,nx,nimg,mirror", ((16, 16, 16, False), (22, 11, 16, True), (80, 48, 48, False), (33, 40, 128, False),
                                               (64, 32, 32, True)))
def test_psf_map_matches_direct_sum(hip_engine, ny, nx, nimg, mirror):
    """One chunk; ragged in both directions plus mirror (k_rays = 22); five panels cut into spans and folded, with a partial
    round of image tiles; the register cap, ragged; api.opd's default shape.  Bundle 2 is an all-NaN map."""
    import torch
    rng = np.random.default_rng(41000 + ny + nx + nimg)
    opd, step, centre = wavefront_maps(rng, 3, ny, nx, mirror, [0.1, 1.0, 0.5])
    opd[2] = np.nan
    want, n = reference_psf(opd, step, nimg, centre, mirror)
    psf, strehl, count = hip_engine.psf_map(opd, step, nimg, DXI, centre=centre, mirror_x=mirror)
    dev = np.abs(psf[:2] - want[:2]).max()
    print(f"psf_map ({ny}, {nx}, {nimg}, {mirror}): worst deviation {dev:.3e}, strehl {strehl[0]:.6f} {strehl[1]:.3e}, N {count}")
    cm.report(f"psf_map {ny} x {nx} nimg {nimg} mirror {mirror}: worst deviation from the direct sum {dev:.2e} (bound {TOL:g})")
    assert dev <= TOL
    assert np.isnan(psf[2]).all() and np.isnan(strehl[2]) and count[2] == 0
    assert np.array_equal(count, n)
    assert np.array_equal(strehl, psf[:, nimg // 2, nimg // 2], equal_nan=True)
    none, only, cnt = hip_engine.psf_map(opd, step, nimg, DXI, centre=centre, mirror_x=mirror, want_psf=False)
    assert none is None and np.array_equal(only, strehl, equal_nan=True) and np.array_equal(cnt, count)
    d = [torch.from_numpy(a).to(torch.device("cuda:0")) for a in (opd, step, centre)]
    torch.cuda.synchronize()
    runs = [hip_engine.psf_map(d[0], d[1], nimg, DXI, centre=d[2], mirror_x=mirror) for _ in range(2)]
    runs.append((runs[0][0],) + hip_engine.psf_map(d[0], d[1], nimg, DXI, centre=d[2], mirror_x=mirror, want_psf=False)[1:])
    hip_engine.ctx.synchronize()
    for dp, ds, dc in runs:                                           # device pointers == host pointers, and run to run
        assert np.array_equal(dp.cpu().numpy(), psf, equal_nan=True) and np.array_equal(ds.cpu().numpy(), strehl, equal_nan=True)
        assert np.array_equal(dc.cpu().numpy(), count)


@pytest.mark.parametrize("nb,ny,nx,nimg,mirror", ((1200, 20, 24, 16, False), (1100, 22, 11, 80, True)))
def test_many_bundles_route(hip_engine, nb, ny, nx, nimg, mirror):
    """More bundles than four workgroups per compute unit: one workgroup per bundle, N divided out at the end, no workspace.
    Every bundle has its own map, step and centre, so an index mix-up between bundles fails.  The second case takes that route
    through the mirrored operand with two image tiles per wave."""
    rng = np.random.default_rng(41415 + nimg)
    opd, step, centre = wavefront_maps(rng, nb, ny, nx, mirror, rng.uniform(0.05, 1.0, size=nb))
    want, n = reference_psf(opd, step, nimg, centre, mirror)
    psf, strehl, count = hip_engine.psf_map(opd, step, nimg, DXI, centre=centre, mirror_x=mirror)
    dev = np.abs(psf - want).max()
    cm.report(f"psf_map, {nb} bundles, nimg {nimg}, mirror {mirror}: worst deviation from the direct sum {dev:.2e} (bound {TOL:g})")
    assert dev <= TOL and np.array_equal(count, n)
    assert np.array_equal(strehl, psf[:, nimg // 2, nimg // 2])
    assert np.array_equal(hip_engine.psf_map(opd, step, nimg, DXI, centre=centre, mirror_x=mirror, want_psf=False)[1], strehl)


def test_conventions(hip_engine):
    """Sign, unit and N^2 normalisation, independently of the reference function: a flat map with a ragged mask peaks at 1; a
    tilt W = 2 a x moves the peak to xi = +2 a; a map sampled from a Zernike wavefront on ort_psf_f64's own grid gives
    ort_psf_f64's image."""
    rng = np.random.default_rng(41999)
    flat = np.where(rng.uniform(size=(1, 19, 27)) < 0.3, np.nan, 0.0)
    assert abs(hip_engine.psf_map(flat, np.array([[0.07, -0.05]]), 16, DXI)[1][0] - 1.0) <= 1e-12
    a, npupil, dp = 0.375, 32, 2.0 / 32
    tilt, step = np.tile(2 * a * np.arange(npupil) * dp, (2, npupil, 1)), np.full((2, 2), dp)
    s = hip_engine.psf_map(tilt, step, 32, DXI, centre=np.array([[2 * a, 0.0], [-2 * a, 0.0]]))[1]
    assert abs(s[0] - 1.0) <= 1e-12 and s[1] < 0.5, s
    x = (2.0 * np.arange(npupil) + 1.0 - npupil) / npupil
    X, Y = np.meshgrid(x, x)
    r2, terms, coef = X * X + Y * Y, ort.zernike_terms(4), np.zeros((1, 14))
    W = np.zeros_like(X)
    for (n, m), c, Z in (((1, 1), 0.2, 2 * X), ((2, 0), -0.15, np.sqrt(3) * (2 * r2 - 1)), ((2, 2), 0.1, np.sqrt(6) * (X * X - Y * Y)),
                         ((3, 1), 0.12, np.sqrt(8) * (3 * r2 - 2) * X), ((4, 0), -0.08, np.sqrt(5) * (6 * r2 * r2 - 6 * r2 + 1))):
        coef[0, terms.index((n, m))] = c
        W += c * Z
    W[r2 > 1.0] = np.nan
    centre = np.array([[0.2, -0.1]])
    want, _ = hip_engine.psf(coef, 4, npupil, 32, DXI, centre=centre)
    got, _, count = hip_engine.psf_map(W[None], np.full((1, 2), dp), 32, DXI, centre=centre)
    assert np.abs(got - want).max() <= TOL and count[0] == (r2 <= 1.0).sum()


def test_psf_opd(hip_engine):
    """api.psf_opd is opd() plus psf_map with the documented steps; the parabola on axis has W = 0, so a Strehl ratio of 1."""
    system = ort.solve(cm.cooke(), cm.COOKE_A, cm.COOKE_H, engine=hip_engine)
    p, s = ort.psf_opd(system, 0.7, engine=hip_engine)
    w = ort.opd(system, 0.7, engine=hip_engine)
    step = np.array([[(w.y[1] - w.y[0]) / w.x[-1], (w.x[1] - w.x[0]) / w.x[-1]]])
    ph, sh, _ = hip_engine.psf_map(w.opd[None], step, 64, DXI, centre=np.zeros((1, 2)), mirror_x=True)
    assert np.array_equal(p, ph[0]) and s == sh[0] and 0.0 < s <= 1.0
    parabola = ort.solve(ort.Layout(cm.parabola_M(), profile=ort.Aspheric), np.full(1, 30.0), 21.0, engine=hip_engine)
    assert abs(ort.psf_opd(parabola, 0.0, k_rays=32, engine=hip_engine)[1] - 1.0) <= 1e-9
    fit = ort.zernike_fit(ort.full_trace(system, 0.0, engine=hip_engine), 10, engine=hip_engine)[0]
    cm.report(f"psf_opd, Cooke H = 0: Strehl from the OPD map {ort.psf_opd(system, 0.0, engine=hip_engine)[1]:.6f}, from the degree-10 "
              f"Zernike fit {ort.psf(fit, 10, engine=hip_engine)[1]:.6f}; H = 0.7 from the map: {s:.6f}")


@pytest.mark.parametrize("kw", (dict(ny=0), dict(nx=2049), dict(nimg=0), dict(nimg=24), dict(nimg=144), dict(dxi=0.0), dict(dxi=-0.1),
                                dict(opd=None), dict(step=None), dict(strehl=None)))
def test_bad_arguments(hip_engine, kw):
    z = np.zeros(4096)
    a = dict(ny=4, nx=4, nimg=16, dxi=DXI, opd=z.ctypes.data, step=z.ctypes.data, strehl=z.ctypes.data)
    a.update(kw)
    rc = hip_engine.ctx.lib.ort_psf_map_f64(hip_engine.ctx.h, 1, a["ny"], a["nx"], a["opd"], a["step"], a["nimg"], a["dxi"], None, None,
                                            a["strehl"], None, 0)
    assert rc == -1                                                   # ORT_EINVAL
