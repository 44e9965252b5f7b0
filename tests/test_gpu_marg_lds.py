"""be_marg with its reduced system, frame blocks and landmark tables in LDS (VIO_MARG_LDS = 1, the default where they fit) against the same stage
with them in HBM scratch (VIO_MARG_LDS = 0, be_marg_hbm_kernel).  Only where operands live differs: every sum keeps its terms and their order, the
two stable compactions of the window slide leave the same order list and free stack.  So everything a handle exposes must be the same BITS.

1. the image pipeline over W + 14 frames, three sequences: window, landmarks, status and the prior (test_gpu_batch's knob tests), for the canonical
   configuration, with the extrinsic / td columns estimated, at 256 and 512 marginalisation threads, and for windows of 12 and 20 keyframes
   (whose system does not fit: both runs take the HBM kernel).
2. generated feature-map streams (backend_cases.py) through vio_process_obs, compared after EVERY frame -- the first marginalisation (no prior yet)
   is one of them in every stream -- including the state arrays of the snapshot that hold the landmark tables (lm_order, lm_free, the flags and
   offsets left in lm_pidx / lm_aidx, start / n_obs / depth / is_dynamic) and the prior.  Each stream asserts on the HBM run that it reaches the edge it
   is here for."""
import ctypes as C

import numpy as np
import pytest

import backend_cases as BC
import vio_ct

pytestmark = pytest.mark.gpu

KNOBS = ("VIO_MARG_LDS", "VIO_MARG_THREADS")
STATE_ROWS = ("lm_id", "lm_start", "lm_nobs", "lm_est_flag", "lm_solve_flag", "lm_dyn", "lm_order", "lm_free", "lm_pidx", "lm_aidx", "lm_depth", "lm_obs",
              "prior_r", "prior_x0", "prior_H")


# ------------------------------------------------------------------------------------------------------------- 1. the image pipeline
_frames = {}


def _rendered(P, sc, seq, tf):
    """host-rendered frames are the same for every configuration that shares the synthetic scene: rendered once per session"""
    key = (bytes(sc), seq, float(tf))
    if key not in _frames:
        _frames[key] = P.Synth(sc).render_host(seq, float(tf))
    return _frames[key]


def _drive(P, cfg, sc, seqs, n):
    syn = P.Synth(sc)
    S = len(seqs)
    b = P.VioBatch(cfg, S)
    imu = [syn.imu(s, int(n / sc.cam_rate * sc.imu_rate) + 64) for s in seqs]
    k = [0] * S
    for tf in vio_ct.frame_times(sc, n):
        for i in range(S):
            ti, ai, gi = imu[i]
            k2 = vio_ct.imu_until(ti, k[i], tf, sc.imu_rate)
            if k2 > k[i]:
                b.push_imu(i, ti[k[i]:k2], ai[k[i]:k2], gi[k[i]:k2])
            k[i] = k2
        fr = [_rendered(P, sc, s, tf) for s in seqs]
        b.feed(np.stack([x[0] for x in fr]), np.stack([x[1] for x in fr]), [tf] * S)
    return b


def _status(b, i):
    st = b.status(i)
    return {k: getattr(st, k) for k, _ in st._fields_}


@pytest.mark.parametrize("kw,threads", [(dict(), None), (dict(estimate_extrinsic=1, estimate_td=1), None), (dict(), "256"), (dict(), "512"),
                                        (dict(window_size=12), None), (dict(window_size=20), None)])
def test_lds_resident_marginalisation_equals_the_hbm_one(P, monkeypatch, kw, threads):
    cfg = P.canonical_config(**kw)
    sc = vio_ct.synth_like(cfg)
    n = cfg.window_size + 14
    for k in KNOBS:
        monkeypatch.delenv(k, raising=False)
    if threads is not None:
        monkeypatch.setenv("VIO_MARG_THREADS", threads)
    monkeypatch.setenv("VIO_MARG_LDS", "0")
    ref = _drive(P, cfg, sc, [60, 61, 62], n)
    monkeypatch.setenv("VIO_MARG_LDS", "1")
    alt = _drive(P, cfg, sc, [60, 61, 62], n)
    for i in range(3):
        sr, sa = _status(ref, i), _status(alt, i)
        assert sr["solver_flag"] == 1 and sr["has_prior"] == 1 and sr["iterations_total"] > n - cfg.window_size, sr
        assert sa == sr, (i, sa, sr)
        assert np.array_equal(alt.window(i).view(np.uint64), ref.window(i).view(np.uint64)), (i, float(np.abs(alt.window(i) - ref.window(i)).max()))
        assert np.array_equal(alt.landmarks(i).view(np.uint64), ref.landmarks(i).view(np.uint64)), i
        pr, pa = ref.prior(i), alt.prior(i)
        assert pr is not None and pa is not None
        for x, y in zip(pr, pa):
            assert np.array_equal(np.ascontiguousarray(x).view(np.uint8), np.ascontiguousarray(y).view(np.uint8)), i


# ------------------------------------------------------------------------------------------------------------- 2. generated streams
class DenseScene(BC.CaseScene):
    """CaseScene with `count` base landmarks on a lattice `step` pixels apart (more than the 49 of the 8-pixel lattice) and gentler motion, so that
    few of them ever share a depth pixel; no extras"""

    def __init__(self, cfg, moves, imu_rate, count, step):
        BC.CaseScene.__init__(self, cfg, moves, imu_rate, amp=0.15, rot=0.02)
        m = BC.WIDTH // step - 1
        uv = np.array([(step * (i + 1) + 0.4, step * (j + 1) + 0.4) for j in range(m) for i in range(m)][:count])
        assert len(uv) == count
        self.n_base = count
        z = np.random.RandomState(9).uniform(3.0, 9.0, count)
        Pc = np.stack([(uv[:, 0] - cfg.cx) / cfg.fx * z, (uv[:, 1] - cfg.cy) / cfg.fy * z, z], 1)
        p, R = self.pose(0.0)
        self.L = Pc @ (R @ self.ric).T + (p + R @ self.tic)


def _dense(P, name, count, step):
    cfg = BC.case_config(P, max_cnt=160, max_landmarks=600)
    W = cfg.window_size
    stamps = BC._stamps(W + 10, 5.0)
    sc = DenseScene(cfg, [(stamps[W], stamps[-1] + 2.0, 2.5)], 100.0, count, step)
    st = BC.Stream(name, cfg, sc, stamps, about="%d landmarks anchored in the oldest frame" % count)
    st.frames()
    return st


def _blank(P):
    """a moving stream whose maps on frames 10 .. 10 + W + 1 hold a single observation under a fresh id: every landmark tracked so far loses its
    observations together and one slide drops them all, leaving only the one-observation newcomers of the last frames (at most W + 1).  An EMPTY map,
    which would leave nothing at all, never reaches the back end: vio_process_obs returns at once on it, as the nodelet only queues non-empty maps."""
    cfg, sc, stamps = BC._moving(P, 22, speed=2.5)
    W = cfg.window_size

    def hook(st, fr):
        if 10 <= fr.k < 10 + W + 2:
            st.renew(fr.lm)
            fr.ids = st.ids_of[fr.lm].copy()
            fr.keep(np.arange(len(fr.lm)) < 1)
    st = BC.Stream("blank", cfg, sc, stamps, hooks=[hook], about="a slide that drops every landmark")
    st.frames()
    return st


def _second_new_only(P):
    """standstill_short: its hold is a run of non-keyframes, each marginalising the second-newest frame (md = 6)"""
    return BC.build("standstill_short", P)


STREAMS = {
    "second_new_run": (_second_new_only, None),
    "no_anchor_in_frame_0": (lambda P: BC.build("thin", P), None),
    "f0_above_64": (lambda P: _dense(P, "f0_above_64", 72, 6), None),
    "f0_above_128": (lambda P: _dense(P, "f0_above_128", 140, 4), None),
    "slide_drops_all": (_blank, None),
    "table_full": (lambda P: BC.build("table_full", P), 10),       # (the frames before the overflow; the table is exactly full on the last)
    "remove_failures": (lambda P: BC.build("reappear", P), None),
    "w10_td": (lambda P: BC.build("w10_td", P), None),             # the LDS path's largest layout with the td column of Cl and newpresent in use
}


def _run(P, st, upto):
    b = P.VioBatch(st.cfg, 1)
    lay = {name: (off, nbytes) for name, kind, nbytes, off in b.snapshot_layout()}
    h0 = C.sizeof(P.SnapshotHeader)
    out = []
    for stamp, ids, obs, depth, (ti, ai, gi) in st.frames()[:upto]:
        if len(ti):
            b.push_imu(0, ti, ai, gi)
        b.process_obs(0, ids, obs, depth, stamp)
        blob = b.save([0])[0]
        pr = b.prior(0)
        out.append(dict(status=_status(b, 0), window=b.window(0).copy(), lm=b.landmarks_ex(0).copy(),
                        prior=None if pr is None else [np.ascontiguousarray(x).copy() for x in pr],
                        state={k: blob[h0 + lay[k][0]:h0 + lay[k][0] + lay[k][1]].copy() for k in STATE_ROWS}))
    cap = b.capacity()
    b.close()
    return out, cap


_anchored = BC.anchored


def _reaches(name, st, ref, cap):
    """the edge the stream is here for, on the run with the tables in HBM"""
    marg_old = [k for k in range(1, len(ref)) if ref[k]["status"]["solver_flag"] == 1 and ref[k - 1]["status"]["solver_flag"] == 1 and
                ref[k]["status"]["marginalization_flag"] == 0]
    first = min(k for k in range(len(ref)) if ref[k]["status"]["has_prior"])
    assert ref[first - 1]["status"]["has_prior"] == 0                       # every stream: the first marginalisation has no prior
    if name == "second_new_run":
        flags = [r["status"]["marginalization_flag"] for r in ref if r["status"]["has_prior"]]
        assert max(len(run) for run in "".join("n" if f else "o" for f in flags).split("o")) >= 5, flags
    elif name == "no_anchor_in_frame_0":
        assert any(ref[k - 1]["status"]["has_prior"] and np.count_nonzero(ref[k - 1]["lm"][:, 1] == 0) == 0 for k in marg_old)
    elif name == "f0_above_64":
        assert any(64 < _anchored(ref[k - 1]) <= 96 for k in marg_old), [_anchored(ref[k - 1]) for k in marg_old]
    elif name == "f0_above_128":
        assert any(128 < _anchored(ref[k - 1]) <= 160 for k in marg_old), [_anchored(ref[k - 1]) for k in marg_old]
    elif name == "slide_drops_all":
        W = st.cfg.window_size
        nl = [r["status"]["n_landmarks"] for r in ref]
        def tracked(k):                                                         # ids of frame k's table with two or more observations
            return ref[k]["lm"][ref[k]["lm"][:, 2] >= 2, 0]
        assert any(nl[k - 1] >= st.scene.n_base and nl[k] <= W + 1 and len(tracked(k - 1)) >= st.scene.n_base and
                   not np.any(np.isin(tracked(k - 1), ref[k]["lm"][:, 0])) for k in marg_old), nl
    elif name == "table_full":
        full = st.notes["full_frame"]                                           # (be_ingest takes the last free slot there: n_free = 0 when be_marg runs)
        assert full == len(ref) - 1 and full in marg_old and ref[full]["status"]["overflow_flags"] == 0
        assert max(r["status"]["n_landmarks"] for r in ref) <= cap["landmarks"]
    elif name == "remove_failures":
        # the slide drops a landmark only when it is left with fewer than two observations: one that vanishes with three or more went by removeFailures
        def dropped_by_failure(k):
            prev, ids = ref[k - 1]["lm"], ref[k]["lm"][:, 0]
            return bool(np.any(~np.isin(prev[:, 0], ids) & (prev[:, 2] >= 3)))
        assert any(dropped_by_failure(k) for k in marg_old)


@pytest.mark.parametrize("name", list(STREAMS))
def test_streams_at_the_edges_of_the_lds_storage(P, monkeypatch, name):
    make, upto = STREAMS[name]
    st = make(P)
    for k in KNOBS:
        monkeypatch.delenv(k, raising=False)
    monkeypatch.setenv("VIO_MARG_LDS", "0")
    ref, cap = _run(P, st, upto)
    monkeypatch.setenv("VIO_MARG_LDS", "1")
    alt, _ = _run(P, st, upto)
    assert ref[-1]["status"]["solver_flag"] == 1 and ref[-1]["status"]["has_prior"] == 1, ref[-1]["status"]
    _reaches(name, st, ref, cap)
    for k, (r, a) in enumerate(zip(ref, alt)):
        assert a["status"] == r["status"], (k, a["status"], r["status"])
        assert np.array_equal(a["window"].view(np.uint64), r["window"].view(np.uint64)), k
        assert np.array_equal(a["lm"].view(np.uint64), r["lm"].view(np.uint64)), k
        assert (a["prior"] is None) == (r["prior"] is None), k
        if r["prior"] is not None:
            for x, y in zip(r["prior"], a["prior"]):
                assert np.array_equal(x.view(np.uint8), y.view(np.uint8)), k
        for row in STATE_ROWS:
            assert np.array_equal(a["state"][row], r["state"][row]), (k, row)
