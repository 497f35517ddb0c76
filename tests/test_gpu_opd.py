"""`ort_opd_grid_f64`: wavefront OPD by optical path length on the device, against a 50-digit trace that keeps the hit points
in 3-D (vertex position + applied sag) and measures the DISTANCES between them — nothing shared with the kernel's excess-path
form but the prescription.  The reference's own error is nil; binary64 rounding predicts eps (|excess| + |spot|) / lambda per
operation, a few 1e-12 waves at millimetres of excess and 587.6 nm.  TOL is 8 x the worst deviation measured over the parity
and parabola cases, rounded up to one digit (condition: never above 1e-7 waves — more would mean a wrong formula).  Measured
worst |W - W_ref| per prescription, in waves: cooke 8.4e-12, tessar 7.0e-12, catadioptric 1.7e-12, aspheric 1.1e-12; statistics
7.0e-12; parabola |W| 7.9e-12, its pv 1.3e-11 — the worst of all: 8 x 1.3e-11 = 1.1e-10, rounded up: 2e-10."""
import functools
import math

import numpy as np
import pytest
from mpmath import hypot, isnan, mpf, sign, sqrt, tan

import opticalraytracing_jl_amd as ort
from opticalraytracing_jl_amd import _capi
from opticalraytracing_jl_amd.engine import Prescription
from oracle import mp_model as mpm
from tests import common as cm

pytestmark = pytest.mark.gpu
TOL, LAM, NAN = 2e-10, 587.5618e-6, float("nan")
NY, NX = 17, 16                       # the full grid: a tile of 256 rays plus one row
KEYS = ("opd", "count", "mean", "rms", "pv")


def _ext(M, focus, K=None, coef=None, ap=None):
    M = np.vstack([np.asarray(M, dtype=np.float64)[:, :3], [math.inf, 0.0, 1.0]]); M[-2, 1] = focus
    return M, K, coef, ap


# authored singlet: row 1 a conic with an odd and two even polynomial terms, row 2 a plain conic; clear apertures on both
ASPH = np.zeros((4, 7)); ASPH[1, 3], ASPH[1, 4], ASPH[1, 6] = 1e-6, 2e-7, -1e-10
# name -> ((rows [R t n], K, coef, clear apertures), stop, a_stop, U, centre of the y axis, half-width of both axes, radius)
CASES = {
    "cooke-axis": (_ext(cm.cooke(), 77.405), 5, 10.3, 0.0, 0.0, 13.0, 90.0),
    "cooke-H1": (_ext(cm.cooke(), 77.405), 5, 10.3, 0.2, -6.0, 13.0, 90.0),
    "tessar-H0.7": (_ext(cm.tessar(), 40.0), 5, 7.63, 0.29, -2.2, 8.5, 45.0),
    "catadioptric": (_ext(cm.catadioptric(), -19.0), 1, 14.0, 0.02, 0.0, 15.0, -40.0),
    "aspheric": (_ext([[math.inf, 0.0, 1.0], [60.0, 8.0, cm.NBK7], [-90.0, 0.0, 1.0]], 70.0, np.array([0.0, -0.8, 0.3, 0.0]), ASPH,
                      np.array([12.5, 10.5, math.inf])), 1, 12.0, 0.05, 0.0, 13.0, 75.0),
}


def setup(name, sy=slice(None), sx=slice(None)):
    """(Prescription, bundle, ref, axes, ny, nx) of a case on the rows sy and columns sx of the full grid."""
    (M, K, coef, ap), stop, a_stop, U, yc, half, radius = CASES[name]
    pres = Prescription(M[:, 0], M[:, 1], M[:, 2], K, None if coef is None else coef[None], ap)
    yax, xax = np.linspace(yc + half, yc - half, NY)[sy], np.linspace(0.0, half, NX)[sx]
    bundle = dict(system=0, stop=stop, U=U, V=0.0, a_stop=a_stop, yaxis_off=0, xaxis_off=len(yax))
    return pres, bundle, dict(y0=yc, x0=0.0, radius=radius), np.concatenate([yax, xax]), len(yax), len(xax)


def mp_ray(M, K, coef, ap, stop, a_stop, U, y, x):
    """One ray at 50 digits -> (E to the image plane, (xf, yf), arriving slopes (v, u), last index), or None: full_trace drops it."""
    R, t, n = (mpm._m(M[:, c]) for c in range(3))
    K = [mpf(0)] * len(R) if K is None else mpm._m(K)
    coef = [None if coef is None or not np.any(coef[i]) else mpm._m(list(coef[i])) for i in range(len(R))]
    u, v, y, x = tan(mpf(U)), mpf(0), mpf(float(y)), mpf(float(x))
    k = [a / sqrt(v * v + u * u + 1) for a in (v, u, mpf(1))]
    E, P, zv, sprev, kept = n[0] * (k[0] * x + k[1] * y), (x, y, mpf(0)), mpf(0), mpf(0), True
    for i in range(len(R) - 1):
        g = (v, u)
        y, x = y + u * (t[i] - sprev), x + v * (t[i] - sprev)
        s = mpm.sag3(y, x, u, v, R[i + 1], K[i + 1], coef[i + 1])
        if isnan(s):
            return None
        y, x, zv, sprev = y + s * u, x + s * v, zv + t[i], s
        Pn = (x, y, zv + s)
        E += n[i] * sqrt(sum((a - b) ** 2 for a, b in zip(Pn, P))) * sign(Pn[2] - P[2])
        P = Pn
        kept = kept and not (i == stop - 1 and hypot(x, y) > a_stop) and not (ap is not None and x * x + y * y > mpf(ap[i]) ** 2)
        m = mpm.tilt3(y, x, R[i + 1], K[i + 1], coef[i + 1]) + [mpf(-1)]
        if not any(isnan(a) for a in m):
            m = [a / sqrt(sum(b * b for b in m)) for a in m]
            eta, c = n[i] / n[i + 1], -sum(a * b for a, b in zip(k, m))
            D = 1 - eta ** 2 * (1 - c ** 2)
            if D >= 0:
                k = [eta * a + (eta * c - sqrt(D)) * b for a, b in zip(k, m)]
        u, v = k[1] / k[2], k[0] / k[2]
    return (E, (x, y), g, n[len(R) - 2]) if kept else None


def mp_path(tr, centre, radius):
    """E of a traced ray up to the reference sphere about `centre`, or None when it does not meet the sphere."""
    E, (x, y), (gv, gu), nlast = tr
    wx, wy, h2 = x - centre[0], y - centre[1], 1 + gu * gu + gv * gv; wg = wx * gv + wy * gu
    disc = wg ** 2 - h2 * (wx ** 2 + wy ** 2 - mpf(radius) ** 2)
    return None if disc < 0 else E + nlast * (-wg - sign(mpf(radius)) * sqrt(disc)) / h2 * sqrt(h2)


@functools.lru_cache(maxsize=None)
def reference(name):
    """W of every node of the full grid as mpf (None: rejected), chief-ray referenced.  Computed once per case."""
    sysm, stop, a_stop, U, yc, half, radius = CASES[name]
    axes, tr = setup(name)[3], mp_ray(*sysm, stop, a_stop, U, yc, 0.0)
    Eref, W = mp_path(tr, tr[1], radius), np.full((NY, NX), None, dtype=object)
    for iy, ix in np.ndindex(NY, NX):
        r = mp_ray(*sysm, stop, a_stop, U, axes[iy], axes[NY + ix])
        E = None if r is None else mp_path(r, tr[1], radius)
        W[iy, ix] = None if E is None else (Eref - E) / mpf(LAM)
    return W


GRIDS = {"1x1": (slice(5, 6), slice(3, 4)), "16x16": (slice(0, 16), slice(None)), "17x16": (slice(None), slice(None))}   # one interior node; exactly one tile; a tile plus one row


@pytest.mark.parametrize("grid", GRIDS)
@pytest.mark.parametrize("name", CASES)
def test_parity_with_the_50_digit_paths(hip_engine, name, grid):
    """NaN pattern, count, W and the statistics against the reference; status bit for bit that of ort_trace_grid_f64."""
    pres, bundle, ref, axes, ny, nx = setup(name, *GRIDS[grid])
    want = reference(name)[GRIDS[grid]]
    got = hip_engine.opd_grid(pres, [bundle], [ref], axes, ny, nx, LAM, want_status=True)[0]
    assert np.array_equal(got["status"].ravel(), hip_engine.grid(pres, [bundle], axes, ny, nx, history=False)["status"])
    assert np.array_equal(np.isnan(got["opd"]), np.array([[w is None for w in row] for row in want]))
    v = [w for w in want.ravel() if w is not None]; mean = sum(v) / len(v); assert int(got["count"]) == len(v)
    stats = dict(mean=mean, rms=sqrt(sum((w - mean) ** 2 for w in v) / len(v)), pv=max(v) - min(v))
    dev = max(abs(float(mpf(float(g)) - w)) for g, w in zip(got["opd"].ravel(), want.ravel()) if w is not None)
    dst = max(abs(float(mpf(float(got[k])) - s)) for k, s in stats.items())
    cm.report(f"opd {name} {grid}: worst |W - W_ref| {dev:.2e}, statistics {dst:.2e} waves (rms {float(stats['rms']):.4g}; bound {TOL:g})")
    assert dev <= TOL and dst <= TOL


def test_parabola_has_no_aberration(hip_engine):
    """First principles, through the public interface: a parabola images a collimated axial beam without aberration, so with
    the sphere about the focus (the axial reference ray's own hit) W = 0 for every ray the stop passes, whatever its height —
    no reference needed.  Mirror space: negative index, thickness and radius.  (32, 16): two tiles."""
    layout = ort.Layout(cm.parabola_M(), profile=ort.Aspheric)
    w = ort.opd(ort.solve(layout, np.full(1, 30.0), 21.0, engine=hip_engine), 0.0, 32, engine=hip_engine)
    live = ~np.isnan(w.opd); dev = np.abs(w.opd[live]).max()
    cm.report(f"opd parabola: {w.count} rays, worst |W| {dev:.2e} waves, pv {w.pv:.2e} (bound {TOL:g})")
    assert w.opd.shape == (32, 16) and w.count == live.sum() > 350 and dev <= TOL and w.pv <= TOL and w.rms <= TOL


def test_bundles_of_one_call_stand_alone(hip_engine):
    """Three systems of one batch: a stop that passes nothing (count 0), a reference ray launched outside the stop (count -1, all
    NaN), and cooke-H1, whose numbers equal, bit for bit, those of the bundle called alone — host or device pointers, run after run."""
    import torch
    pres, bundle, ref, ax, _, _ = setup("cooke-H1")
    three = Prescription(np.tile(pres.R, (3, 1)), np.tile(pres.t, (3, 1)), np.tile(pres.n, (3, 1)))
    axes = np.concatenate([ax[:NY], ax[NY:] + 0.5, ax, ax])                       # bundle 0 has no node on its reference ray
    bundles = [dict(bundle, system=s, yaxis_off=s * (NY + NX), xaxis_off=s * (NY + NX) + NY) for s in range(3)]
    bundles[0].update(U=0.0, a_stop=0.0)
    refs = [dict(ref, y0=0.0), dict(ref, y0=40.0), ref]
    alone = hip_engine.opd_grid(pres, [bundle], [ref], ax, NY, NX, LAM)[0]
    res = hip_engine.opd_grid(three, bundles, refs, axes, NY, NX, LAM)
    assert int(res[0]["count"]) == 0 and int(res[1]["count"]) == -1
    assert all(np.isnan(r["opd"]).all() and all(np.isnan(r[k]) for k in KEYS[2:]) for r in res[:2])
    assert all(np.array_equal(res[2][k], alone[k], equal_nan=True) for k in KEYS)
    dax = torch.from_numpy(axes).to("cuda:0"); torch.cuda.synchronize()
    for _ in range(2):
        dev = hip_engine.opd_grid(three, bundles, refs, dax, NY, NX, LAM)
        hip_engine.ctx.synchronize()
        assert all(np.array_equal(np.asarray(r[k]), d[k].cpu().numpy(), equal_nan=True) for r, d in zip(res, dev) for k in KEYS)


@pytest.mark.parametrize("change", [dict(sys=None), dict(bundles=None), dict(refs=None), dict(axes=None), dict(count=None), dict(rms=None),
                                    dict(lam=0.0), dict(lam=NAN), dict(radius=0.0), dict(radius=math.inf), dict(stop=0),
                                    dict(flags=_capi.ORT_RAYBASIS), dict(ny=0), dict(nx=NX + 1), dict(system=1)],
                         ids=lambda c: "-".join(f"{k}={v}" for k, v in c.items()))
def test_bad_arguments(hip_engine, change):
    """Every ORT_EINVAL of the header, each as one change to a call that is accepted."""
    pres, bundle, ref, axes, _, _ = setup("cooke-axis")
    count, rms, sysd = np.zeros(1, dtype=np.int64), np.zeros(1), hip_engine.system(pres)
    def call(**ch):
        barr = _capi.make_bundles([dict(bundle, **{k: ch.pop(k) for k in ("stop", "system") if k in ch})])
        rarr = (_capi.ort_opd_ref * 1)(_capi.ort_opd_ref(0.0, 0.0, NAN, NAN, ch.pop("radius", 90.0)))
        a = dict(dict(sys=sysd.h, bundles=barr, refs=rarr, axes=axes.ctypes.data, ny=NY, nx=NX, lam=LAM, count=count.ctypes.data,
                      rms=rms.ctypes.data, flags=0), **ch)
        return hip_engine.ctx.lib.ort_opd_grid_f64(hip_engine.ctx.h, a["sys"], 1, a["bundles"], a["refs"], a["axes"], axes.size, a["ny"],
                                                   a["nx"], a["lam"], None, None, a["count"], None, a["rms"], None, a["flags"])
    assert call() == 0 and call(**change) == -1
