"""KANNALA_BRANDT and MEI camera models on the CPU: vio_stage_host_camera (csrc/camera_model.h) against the numpy restatement of camodocal
(tests/camera_ref.py), MEI with xi = 0 against PINHOLE bit for bit, and the host renderer's ray table."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import camera_ref as cr  # noqa: E402

PINHOLE = dict(fx=604.5821781259577, fy=604.2544712985845, cx=321.2638233484251, cy=239.70969315130674, k1=0.13387871564774004,
               k2=-0.2731913133377051, p1=0.0020296263577681264, p2=-0.00044384544608203714)


def _kb(P, k=None, **over):
    c = dict(cr.KB_LENS)
    if k is not None:
        c.update(k2=k[0], k3=k[1], k4=k[2], k5=k[3])
    c.update(over)
    return c, P.camera_kannala_brandt(*(c[n] for n in P.CAMERA_PARAMS[P.CAMERA_KANNALA_BRANDT]))


def _mei(P, **over):
    c = dict(cr.MEI_LENS)
    c.update(over)
    return c, P.camera_mei(*(c[n] for n in P.CAMERA_PARAMS[P.CAMERA_MEI]))


def _points():
    return np.concatenate([cr.grid(), cr.random_points(800, 7)])


def _check(P, model, params, cam, uv, lift_tol=1e-12, proj_tol=1e-9, R=None):
    ray, un, uvo = P.stage_host_camera(cam, uv, R)
    ref = cr.lift(model, params, uv)
    assert np.abs(ray - ref).max() <= lift_tol, float(np.abs(ray - ref).max())
    assert np.array_equal(un, ray[:, :2] / ray[:, 2:3])
    Rm = np.eye(3) if R is None else np.asarray(R).reshape(3, 3)
    pref = cr.project(model, params, ray @ Rm.T)
    assert np.abs(uvo - pref).max() <= proj_tol, float(np.abs(uvo - pref).max())
    return ray, uvo


def test_abi_version_and_struct_size(P):
    L = P.lib()
    assert L.vio_abi_version() >= 11
    assert L.vio_abi_sizeof(3) == C.sizeof(P.Camera) == 104


@pytest.mark.parametrize("lens", ["kb", "mei"])
def test_test_lenses_match_the_restatement(P, lens):
    params, cam = _kb(P) if lens == "kb" else _mei(P)
    model = int(cam.model)
    uv = _points()
    ray, uvo = _check(P, model, params, cam, uv)
    # project(lift(p)) returns p: 2e-12 px for KANNALA_BRANDT; MEI's 8-step inverse does not fully converge (4.5e-9 px, the reference's lift)
    assert np.abs(uvo - uv).max() <= (1e-10 if lens == "kb" else 1e-8)
    # a rotation between lift and projection, as predictPtsInNextFrame applies it
    a = 0.05
    R = np.array([[np.cos(a), 0, np.sin(a)], [0, 1, 0], [-np.sin(a), 0, np.cos(a)]])
    _check(P, model, params, cam, uv, R=R)


def _g(k, th):
    return th + k[0] * th ** 3 + k[1] * th ** 5 + k[2] * th ** 7 + k[3] * th ** 9


@pytest.mark.parametrize("edge", sorted(cr.KB_EDGE))
def test_kb_edge_lenses(P, edge):
    k = cr.KB_EDGE[edge]
    params, cam = _kb(P, k)
    uv = _points()
    if edge == "three_roots":
        # where two roots (nearly) merge the companion-matrix eigenvalues are complex within sqrt(eps) and the reference's pick is a coin
        # toss: leave out |p_u| within 2e-3 of the local extremes of r(theta) (0.7563 and 0.5459)
        rn = np.hypot((uv[:, 0] - params["u0"]) / params["mu"], (uv[:, 1] - params["v0"]) / params["mv"])
        uv = uv[(np.abs(rn - 0.75632) > 2e-3) & (np.abs(rn - 0.54591) > 2e-3)]
    ray, _ = _check(P, 1, params, cam, uv)
    th = np.arctan2(np.hypot(ray[:, 0], ray[:, 1]), ray[:, 2])
    rn = np.hypot((uv[:, 0] - params["u0"]) / params["mu"], (uv[:, 1] - params["v0"]) / params["mv"])
    if edge == "three_roots":
        band = (rn > 0.56) & (rn < 0.74)
        assert band.sum() > 50
        assert np.all(th[band] < 1.2137)                      # the first of the three roots, below the local maximum of r(theta)
    if edge == "no_root":
        far = rn > 0.87
        assert far.sum() > 50
        assert np.allclose(th[far], rn[far], rtol=0, atol=1e-12)   # the fallback theta = |p_u|
    if edge == "dropped_k5":
        lifted = (-0.01, 0.0, 0.001, 0.0)
        assert np.abs(_g(lifted, th) - rn).max() < 1e-12           # the lift solved the degree-7 polynomial
        assert np.abs(_g(k, th) - rn).max() > 1e-6                 # ... and not the projection's
    if edge == "zero":
        assert np.abs(th - rn).max() < 1e-12


def test_mei_special_cases(P):
    uv = _points()
    for over in (dict(xi=1.0), dict(k1=0.0, k2=0.0, p1=0.0, p2=0.0), dict(xi=1.0, k1=0.0, k2=0.0, p1=0.0, p2=0.0)):
        params, cam = _mei(P, **over)
        _check(P, 2, params, cam, uv)


def test_mei_with_xi_zero_is_pinhole_bit_for_bit(P):
    uv = _points()
    pin = P.Camera()
    pin.model = P.CAMERA_PINHOLE
    for i, n in enumerate(P.CAMERA_PARAMS[P.CAMERA_PINHOLE]):
        pin.p[i] = PINHOLE[n]
    mei = P.camera_mei(0.0, PINHOLE["k1"], PINHOLE["k2"], PINHOLE["p1"], PINHOLE["p2"], PINHOLE["fx"], PINHOLE["fy"], PINHOLE["cx"],
                       PINHOLE["cy"])
    a = 0.03
    R = np.array([[np.cos(a), -np.sin(a), 0], [np.sin(a), np.cos(a), 0], [0, 0, 1]]) @ \
        np.array([[1, 0, 0], [0, np.cos(a), -np.sin(a)], [0, np.sin(a), np.cos(a)]])
    rp, up, op = P.stage_host_camera(pin, uv, R)
    rm, um, om = P.stage_host_camera(mei, uv, R)
    assert np.array_equal(rp, rm) and np.array_equal(up, um) and np.array_equal(op, om)
    assert np.all(rm[:, 2] == 1.0)
    _check(P, 0, PINHOLE, pin, uv)


@pytest.mark.parametrize("lens", ["kb", "mei"])
def test_host_ray_table_is_the_lift(P, lens):
    """vio_synth_render_host_camera renders deterministically through its own camera, and its ray table (build_rays: float32 of
    camera_model.h's x / z, y / z, the lift vio_stage_host_camera runs) is the restatement's lift to within one float32 rounding."""
    params, cam = _kb(P) if lens == "kb" else _mei(P)
    sc = P.default_synth()
    syn = P.Synth(sc)
    g, d = syn.render_host(3, 2.0, camera=cam)
    g2, d2 = syn.render_host(3, 2.0, camera=cam)
    assert np.array_equal(g, g2) and np.array_equal(d, d2)
    g0, d0 = syn.render_host(3, 2.0)
    assert not np.array_equal(g, g0)   # another camera, other rays
    # the table itself, through the shared lift: float32 of the restatement's x / z, y / z
    uv = cr.grid(step=8)
    ref = cr.lift(int(cam.model), params, uv)
    _, un, _ = P.stage_host_camera(cam, uv)
    assert np.abs(un - ref[:, :2] / ref[:, 2:3]).max() < 1e-11
    np.testing.assert_array_max_ulp(un.astype(np.float32), (ref[:, :2] / ref[:, 2:3]).astype(np.float32), maxulp=1)


def test_pinhole_camera_renders_what_the_config_renders(P):
    sc = P.default_synth()
    syn = P.Synth(sc)
    cam = P.camera_pinhole(sc)
    g, d = syn.render_host(5, 2.5, camera=cam)
    g0, d0 = syn.render_host(5, 2.5)
    assert np.array_equal(g, g0) and np.array_equal(d, d0)


# ---------------------------------------------------------------------------------------------------------------- configuration files
_BASE = """%YAML:1.0
image_width: 640
image_height: 480
"""
_KB_YAML = _BASE + """model_type: kannala_brandt
projection_parameters:
   k2: -0.012
   k3: 0.0035
   k4: -0.0007
   k5: 0.00005
   mu: 330.0
   mv: 330.0
   u0: 321.26
   v0: 239.71
"""
_MEI_YAML = _BASE + """model_type: MEI
mirror_parameters:
   xi: 1.2
distortion_parameters:
   k1: -0.12
   k2: 0.02
   p1: 0.0002
   p2: -0.0003
projection_parameters:
   gamma1: 900.0
   gamma2: 900.0
   u0: 321.26
   v0: 239.71
"""
_PIN_YAML = _BASE + """model_type: PINHOLE
distortion_parameters:
   k1: 0.1
   k2: -0.2
   p1: 0.001
   p2: -0.002
projection_parameters:
   fx: 600.0
   fy: 601.0
   cx: 320.0
   cy: 240.0
"""


@pytest.fixture(scope="module")
def io():
    import importlib
    return importlib.import_module("vins-rgbd-fast_amd.dataio")


def test_kb_and_mei_files_parse_to_their_camera(P, io):
    _, e = io.config_from_yaml(_KB_YAML, P)
    assert e["camera"] == _kb(P)[1] and e["notes"] == []
    _, e = io.config_from_yaml(_MEI_YAML, P)
    assert e["camera"] == _mei(P)[1] and e["notes"] == []
    c, e = io.config_from_yaml(_PIN_YAML, P)
    assert e["camera"] is None and (c.fx, c.cy, c.k2) == (600.0, 240.0, -0.2)


@pytest.mark.parametrize("text,drop", [(_KB_YAML, "   k5: 0.00005\n"), (_KB_YAML, "   mv: 330.0\n"), (_MEI_YAML, "   xi: 1.2\n"),
                                       (_MEI_YAML, "   gamma2: 900.0\n"), (_MEI_YAML, "   p1: 0.0002\n")])
def test_incomplete_camera_files(P, io, text, drop):
    bad = text.replace(drop, "")
    with pytest.raises(ValueError):
        io.config_from_yaml(bad, P)
    c, e = io.config_from_yaml(bad, P, strict=False)
    assert len(e["notes"]) == 1 and e["camera"] is None
    assert c.width == 640


def test_scaramuzza_is_refused(P, io):
    with pytest.raises(ValueError):
        io.config_from_yaml(_BASE + "model_type: SCARAMUZZA\n", P)


def test_batch_of_pinhole_kb_and_mei_files(P, io, tmp_path):
    paths = []
    for name, text in (("pin", _PIN_YAML), ("kb", _KB_YAML), ("mei", _MEI_YAML)):
        p = tmp_path / (name + ".yaml")
        p.write_text(text)
        paths.append(str(p))
    cfg, cals, extras = io.batch_config_from_yamls(paths, P)
    assert [e["camera"] for e in extras] == [None, _kb(P)[1], _mei(P)[1]]
    assert cals[0].fx == 600.0 and len(cals) == 3
