"""The high-precision definitions of tests/pose_ref.py checked against themselves, and the CPU twins of the device pose solvers (the host
copy of csrc/dyninit_host.cpp, the oracle) held to the tolerances that tests/test_gpu_pose_edges.py then asks of the device: if a twin, which
runs the same formulas in IEEE double, does not stay inside a bound, the bound is wrong, not the device."""
import mpmath as mp
import numpy as np
import pytest

import excalib_ref as X
import pose_cases as PC
import pose_ref as PR


@pytest.fixture(scope="module")
def twins(P, orc):
    PC.bind(orc)
    return {"oracle": (orc.ovio_rodrigues, orc.ovio_solve_pnp_trace), "host": (P.lib().vio_stage_host_rodrigues, P.lib().vio_stage_host_pnp_trace)}


# ------------------------------------------------------------------------------------------------------------- the definitions
def test_dexp_closed_form_matches_central_difference():
    for r in ([0.3, -0.5, 0.8], [1e-9, 2e-9, -1e-9], [0.0, 0.0, 3.0], [2.0, -2.2, 1.0], [4.0, 3.0, -5.0]):
        r = [mp.mpf(x) for x in r]
        d = PR.dexp_mp(r)
        h = mp.mpf("1e-20")
        for i in range(3):
            rp, rm = list(r), list(r)
            rp[i] += h; rm[i] -= h
            fd = (PR.exp_mp(rp) - PR.exp_mp(rm)) / (2 * h)
            assert max(abs(fd[a, b] - d[i][a, b]) for a in range(3) for b in range(3)) < mp.mpf("1e-28"), (r, i)
    G = PR.dexp_mp([0, 0, 0])
    assert G[0][2, 1] == 1 and G[1][0, 2] == 1 and G[2][1, 0] == 1


def test_log_inverts_exp():
    for r in ([0.3, -0.5, 0.8], [1e-12, 0, 0], [0, 0, 0], [0.0, 3.1, 0.0], [1.0, 2.0, -2.0]):
        back = PR.log_mp(PR.exp_mp([mp.mpf(x) for x in r]))
        assert max(abs(a - mp.mpf(b)) for a, b in zip(back, r)) < mp.mpf("1e-35"), r
    k = [mp.mpf(3) / 5, 0, mp.mpf(4) / 5]
    back = PR.log_mp(PR.exp_mp([mp.pi * x for x in k]))
    assert max(abs(a - mp.pi * b) for a, b in zip(back, k)) < mp.mpf("1e-35")


# ------------------------------------------------------------------------------------------------------------- cv::Rodrigues twins
@pytest.mark.parametrize("which", ["oracle", "host"])
def test_rodrigues_twins_stay_inside_the_tolerances(twins, which):
    PC.check_exp(twins[which][0])
    PC.check_log(twins[which][0], twins["oracle"][0])


def test_log_cases_reach_both_sides_of_every_threshold():
    by = {name: PC.log_branch(R)[0] for name, R, _ in PC.log_cases()}
    for ax in PC.axes():
        assert by[ax + "@9e-6"] == "zero" and by[ax + "@1.1e-5"] == "regular", ax
        assert by[ax + "@pi-1.1e-5"] == "regular" and by[ax + "@pi-9e-6"] == "pi" and by[ax + "@pi"] == "pi", ax
    th2 = [float(r @ r) for _, r in PC.exp_cases()]
    assert any(0 < x < 1e-24 for x in th2) and any(1e-24 <= x < 2e-24 for x in th2)


# ------------------------------------------------------------------------------------------------------------- solvePnP
@pytest.mark.parametrize("name", list(PC.pnp_cases()))
def test_pnp_case_takes_its_path_on_the_cpu_twins(twins, name):
    c = PC.pnp_cases()[name]
    ro, to, tro = PC.call_pnp(twins["oracle"][1], c)
    rh, th, trh = PC.call_pnp(twins["host"][1], c)
    assert c["expect"](tro), (name, c["about"], tro)
    assert trh == tro, (name, tro, trh)
    if not tro[3]:
        assert not np.isfinite(np.r_[ro, to]).all() and not np.isfinite(np.r_[rh, th]).all()
        return
    if name == "z_zero":
        assert np.array_equal(ro, c["rvec0"]) and np.array_equal(to, c["tvec0"]) and np.array_equal(rh, ro) and np.array_equal(th, to)
        return
    if tro[0] == 20:
        assert PC.pnp_cost(c, rh, th) <= PC.pnp_cost(c, ro, to) * (1 + 1e-9)
    else:
        assert np.abs(PC.rot(rh) - PC.rot(ro)).max() < 1e-7 and np.abs(th - to).max() < 1e-7
    if c["noise_free"]:
        assert PC.truth_distance(c, rh, th) <= 2 * PC.truth_distance(c, ro, to), name


def test_zero_start_stops_by_the_published_norm(twins):
    """cvNorm(param, prev, CV_RELATIVE_L2) = |param - prev| / (|prev| + DBL_EPSILON): with prev = 0 and a zero step the ratio is 0 and the
    solve stops after its first iteration; with prev = 0 and a real step it is huge and the solve goes on"""
    cs = PC.pnp_cases()
    for fn in (twins["oracle"][1], twins["host"][1]):
        assert PC.call_pnp(fn, cs["zero_start_zero_truth"])[2] == (1, 0, -4, 1)
        r, t, tr = PC.call_pnp(fn, cs["zero_start_small_motion"])
        assert tr[0] >= 2 and PC.truth_distance(cs["zero_start_small_motion"], r, t) < 1e-6


# ------------------------------------------------------------------------------------------------------------- solveRelativeR
def test_extended_restatement_equals_the_old_one_on_the_old_cases(P, orc):
    """the cases of test_gpu_ex_calib.test_stage_relative_r_matches_restatement: the oracle's RANSAC keeps every correspondence there, and the
    restatement with that mask is the old restatement bit for bit"""
    rs = np.random.RandomState(11)
    for n in (9, 14, 15, 150, 300):
        for noise in (0.0, 0.5):
            for m in range(4):
                R = X.rodrigues(rs.normal(0, 0.15, 3))
                t = rs.normal(0, 0.3, 3)
                co = PC._relative_r_case(rs, n, noise, R, t)
                mask = PR.ransac_mask(orc, P, co)
                assert mask.all(), (n, noise, m)
                old, d_old = X.solve_relative_r(co, detail=True)
                new, d = PR.solve_relative_r(co, mask)
                assert np.array_equal(old, new) and d["win"] == d_old["win"] and (max(d["cnt"][:2]), max(d["cnt"][2:])) == d_old["votes"]


def test_relative_r_cases_reach_their_branches(P, orc):
    cs = PC.relative_r_cases()
    near = []
    for name, c in cs.items():
        co = c["co"]
        mask = PR.ransac_mask(orc, P, co) if len(co) >= 9 else None
        R, d = PR.solve_relative_r(co, mask)
        if d["F22"] is not None and abs(abs(d["F22"]) - X.FLT_EPS) <= 10 * X.FLT_EPS:
            near.append(name)
        if name == "wide_angle":
            assert 300 - d["inliers"] >= 20 and d["inliers"] >= 200, d["inliers"]
        elif name == "left_identical" or len(co) < 9:
            assert d["found"] == 0 and np.array_equal(R, np.eye(3))
        else:
            assert d["found"] == 1 and d["inliers"] == len(co), name
        if c["truth"] is not None:
            assert X.rot_angle_deg(R, c["truth"]) < 1e-3, name
    # only there may a sign change of F swap the labels R1 / R2 between two implementations
    assert set(near) <= {"translation_sideways_noise0", "translation_forward_noise0"}, near
    assert {cs[k]["exact_translation"] for k in near} <= {True}
