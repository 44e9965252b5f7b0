"""vio_publish_all (pubPointCloud + pubKeyframe for the whole batch in one launch) against its definition in
tests/publish_ref.py: the stage entry on random tables at the edges of the list walk, live handles over the streams of
tests/publish_cases.py after every frame, a batch against solo runs, the HBM destination, read-only behaviour, an image-fed handle with tracker
lag 1 and the split marginalisation, the loop-closure chain from a published keyframe, and the C++ mirror.

Bit for bit throughout, with one exception: a live handle's world points.  There the definition has the window's quaternion, not Rs, so the two
sides differ by the roundings of matrix -> quaternion -> matrix and of the two affine steps.  The bar per coordinate is
32 * 2^-53 * (|P| + |R| (|ric| |pc| + |tic|)), the sum over the absolute values of the terms (8 roundings for each conversion, 4 for each affine
step, with slack); the largest observed ratio to it is printed and recorded in DESIGN.md section 6f."""
import os
import subprocess

import numpy as np
import pytest

import backend_cases as BC
import publish_cases as PC
import publish_ref as PR
import vio_ct

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EPS = 2.0 ** -53
BLOCK = 256
NL = 2 * BLOCK + 8
_solo = {}


def bits(a):
    return np.ascontiguousarray(a, np.float64).view(np.uint64)


def same_bits(a, b):
    a, b = np.ascontiguousarray(a, np.float64), np.ascontiguousarray(b, np.float64)
    return a.shape == b.shape and np.array_equal(bits(a), bits(b))


def R_to_quat(m):
    """dm::R2q (csrc/dmath.h: Eigen's Quaternion(Matrix3)) operation for operation: (w, x, y, z)"""
    m = np.asarray(m, np.float64).reshape(3, 3)
    t = np.float64(m[0, 0] + m[1, 1] + m[2, 2])
    if t > 0:
        t = np.sqrt(t + 1.0)
        w = 0.5 * t
        t = 0.5 / t
        return np.array([w, (m[2, 1] - m[1, 2]) * t, (m[0, 2] - m[2, 0]) * t, (m[1, 0] - m[0, 1]) * t])
    i = 0
    if m[1, 1] > m[0, 0]:
        i = 1
    if m[2, 2] > m[i, i]:
        i = 2
    j, k = (i + 1) % 3, (i + 2) % 3
    t = np.sqrt(m[i, i] - m[j, j] - m[k, k] + 1.0)
    q = np.zeros(4)
    q[1 + i] = 0.5 * t
    t = 0.5 / t
    q[0] = (m[k, j] - m[j, k]) * t
    q[1 + j] = (m[j, i] + m[i, j]) * t
    q[1 + k] = (m[k, i] + m[i, k]) * t
    return q


# ------------------------------------------------------------------------------------------------------------- the stage entry
def random_tables(rs, W, half_turn=False):
    """NL slots with every combination of the flags: start anywhere in the window (a fifth in frame 0), 1 .. W + 1 - start observations (a third cut to 1 .. 3), solve_flag 0 / 1 / 2, dynamic
    or not, a first depth of zero for a third of them; every observation row filled, ids distinct, lm_order a random permutation"""
    W1 = W + 1
    t = dict(lm_order=rs.permutation(NL).astype(np.int32), lm_id=rs.permutation(100000)[:NL].astype(np.int32),
             lm_start=rs.randint(0, W1, NL).astype(np.int32), lm_solve_flag=rs.randint(0, 3, NL).astype(np.int32),
             lm_dyn=(rs.uniform(size=NL) < 0.25).astype(np.int32), lm_depth=rs.uniform(0.5, 9.0, NL), lm_obs=rs.uniform(-1.0, 1.0, (NL, W1, 9)))
    t["lm_start"][rs.uniform(size=NL) < 0.2] = 0                                       # (the margin cloud wants start 0 and a short track)
    t["lm_nobs"] = np.array([rs.randint(1, W1 - s + 1) for s in t["lm_start"]], np.int32)
    short = rs.uniform(size=NL) < 0.3
    t["lm_nobs"][short] = np.minimum(t["lm_nobs"][short], rs.randint(1, 4, int(short.sum())))
    t["lm_obs"][:, :, 8] = np.where(rs.uniform(size=(NL, W1)) < 0.33, 0.0, rs.uniform(0.5, 9.0, (NL, W1)))
    t["lm_obs"][:, :, 3:5] = rs.uniform(0.0, 640.0, (NL, W1, 2))
    t["Ps"] = rs.uniform(-5.0, 5.0, (W1, 3))
    Rs = np.stack([BC.X.rodrigues(rs.uniform(-1.0, 1.0, 3) * (np.pi - 1e-3 if half_turn else 1.0)) for _ in range(W1)])
    t["Rs"], t["Headers"] = Rs, 100.0 + np.cumsum(rs.uniform(0.05, 0.3, W1))
    t["ric"], t["tic"] = BC.X.RIC_TRUE.copy(), BC.X.TIC_TRUE.copy()
    return t


def definition_of(t, W, n_lm, ring, flags):
    """the definition's inputs from the tables: landmarks_ex rows in list order (slots outside [0, NL) are not landmarks), the window and the
    observations filed under window frame W-2"""
    W1 = W + 1
    rows, fed = [], {}
    for k in range(min(max(n_lm, 0), NL)):
        s = int(t["lm_order"][k])
        if not 0 <= s < NL:
            continue
        st, no = int(t["lm_start"][s]), int(t["lm_nobs"][s])
        o0, ob = t["lm_obs"][s, (st + ring) % W1], t["lm_obs"][s, (st + max(no, 1) - 1 + ring) % W1]
        rows.append([t["lm_id"][s], st, no, t["lm_depth"][s], 0, t["lm_solve_flag"][s], t["lm_dyn"][s], o0[0], o0[1], o0[2], o0[8], ob[8]])
        fed[int(t["lm_id"][s])] = t["lm_obs"][s, (W - 2 + ring) % W1, :7]
    win = np.zeros((W1, 17))
    win[:, 0:3], win[:, 16] = t["Ps"], t["Headers"]
    win[:, 3:7] = [R_to_quat(R) for R in t["Rs"]]
    status = dict(solver_flag=flags[0], marginalization_flag=flags[1], processed=flags[2])
    return PR.publish(np.array(rows, np.float64).reshape(-1, 12), win, np.concatenate([t["tic"], t["ric"].reshape(-1), [0.0]]), status,
                      {float(t["Headers"][W - 2]): fed}, Rs=t["Rs"])


_defs = {}


def check_stage(P, t, W, n_lm, ring, flags, cap, lists=(True, True, True)):
    key = (id(t), W, n_lm, ring, flags)           # (the definition does not depend on cap: computed once per table and walk)
    if key not in _defs:
        _defs[key] = (t, definition_of(t, W, n_lm, ring, flags))
    want = _defs[key][1]
    counts, pose, cloud, margin, kf = P.stage_publish(t, W, n_lm, ring, flags, cap, lists=lists)
    where = (W, n_lm, ring, flags, cap)
    assert np.array_equal(counts, want[0]), (where, counts, want[0])
    if want[1] is None:
        assert np.isnan(pose).all(), where
    else:
        assert same_bits(pose, want[1]), (where, pose, want[1])
    for got, ref, on in zip((cloud, margin, kf), want[2:5], lists):
        if not on:
            assert got is None
            continue
        m = min(len(ref), cap)
        assert same_bits(got[:m], ref[:m]), (where, got.shape[1])
        assert np.isnan(got[m:]).all(), (where, "rows at and beyond min(count, cap) were written")
    return want[0]


@pytest.mark.parametrize("W", [4, 10, 20])
def test_stage_entry_equals_the_definition_bit_for_bit(P, W):
    rs = np.random.RandomState(100 + W)
    t = random_tables(rs, W)
    flag_sets = [(a, b, c) for a in (0, 1) for b in (0, 1) for c in (0, 1)]
    seen_kf = 0
    for i, n_lm in enumerate((0, 1, 63, 64, 65, BLOCK - 1, BLOCK, BLOCK + 1, 2 * BLOCK + 1, NL)):
        for ring in (0, 1, W):
            flags = (1, 0, 1) if (i + ring) % 2 == 0 else flag_sets[(i + ring) % 8]
            counts = check_stage(P, t, W, n_lm, ring, flags, NL)
            seen_kf += int(counts[2] > 0)
            caps = {0, 1}
            for c in counts[:3]:
                caps |= {int(c) - 1, int(c), int(c) + 1}
            for cap in sorted(c for c in caps if 0 <= c < NL):
                check_stage(P, t, W, n_lm, ring, flags, cap)
    for flags in flag_sets:                      # every combination of the three keyframe conditions on the full list
        check_stage(P, t, W, NL, 1, flags, NL)
    assert seen_kf >= 10
    full = definition_of(t, W, NL, 0, (1, 0, 1))[0]
    assert full[0] > 40 and full[1] > 2 and full[2] > 8, full   # the lists are not trivially short


def test_stage_entry_counts_null_lists_and_skips_what_is_not_a_landmark(P):
    W = 10
    rs = np.random.RandomState(7)
    t = random_tables(rs, W, half_turn=True)      # rotations near pi: the other branch of the matrix -> quaternion routine
    assert any(R[0, 0] + R[1, 1] + R[2, 2] <= 0 for R in t["Rs"])
    for lists in ((False, True, True), (True, False, True), (True, True, False), (False, False, False)):
        check_stage(P, t, W, NL, 3, (1, 0, 1), 40, lists=lists)
    for f in range(W + 1):                         # the pose row through both branches of the conversion
        t2 = dict(t, Rs=np.roll(t["Rs"], f, axis=0))
        check_stage(P, t2, W, 65, 0, (1, 0, 1), NL)
    # slots outside [0, NL) in the list are skipped, an n_lm beyond NL is clamped: never dereferenced
    bad = dict(t, lm_order=t["lm_order"].copy())
    bad["lm_order"][[3, 64, 300]] = (-1, NL, 2 ** 31 - 1)
    a = check_stage(P, bad, W, NL, 2, (1, 0, 1), NL)
    b = check_stage(P, bad, W, NL + 1000, 2, (1, 0, 1), NL)
    c = check_stage(P, bad, W, -5, 2, (1, 0, 1), NL)
    assert np.array_equal(a, b) and not c[:3].any()


# ------------------------------------------------------------------------------------------------------------- live handles
def status_dict(st):
    return {k: getattr(st, k) for k, _ in st._fields_}


def check_live(b, s, pub, mirror, worst, where, obs=True):
    """publish() of slot s against the definition fed from the same handle's per-sequence getters"""
    W = b.W
    lm, win, ex, st = b.landmarks_ex(s), b.window(s), b.extrinsic(s), b.status(s)
    fed = mirror.fed_at(lm, win, W - 2) if mirror is not None else NoObs()
    counts, pose, cloud, margin, kf, b_cloud, b_margin, b_kf = PR.publish(lm, win, ex, st, fed, with_bounds=True)
    assert np.array_equal(pub["counts"][s], counts), (where, pub["counts"][s], counts)
    if pose is None:
        assert not pub["kf_pose"][s].any(), where
    else:
        assert same_bits(pub["kf_pose"][s], pose), (where, pub["kf_pose"][s], pose)
        assert same_bits(pub["kf_pose"][s], np.concatenate([[win[W - 2, 16]], win[W - 2, 0:7]])), where
    for name, ref, bound in (("cloud", cloud, b_cloud), ("margin", margin, b_margin), ("kf_points", kf, b_kf)):
        got = pub[name][s]
        n = len(ref)
        assert not got[n:].any(), (where, name)
        if n == 0:
            continue
        ratio = np.abs(got[:n, 0:3] - ref[:, 0:3]) / (32.0 * EPS * bound)
        worst[0] = max(worst[0], float(ratio.max()))
        assert ratio.max() <= 1.0, (where, name, float(ratio.max()))
        if name == "kf_points":
            assert same_bits(got[:n, 7], ref[:, 7]), (where, "ids / order")
            if obs:
                assert same_bits(got[:n, 3:7], ref[:, 3:7]), (where, "x y u v")


class NoObs(dict):
    """stands in for the fed maps where only counts, order, ids and points are compared"""

    def __missing__(self, key):
        return NoObs.Row()

    class Row(dict):
        def __missing__(self, key):
            return np.zeros(7)


def run_solo(P, name):
    """a one-sequence handle over the stream through vio_process_obs_batch; after every offer publish() is checked against the definition.
    Returns the publications, per offer"""
    if name in _solo:
        return _solo[name]
    st = PC.build(name, P)
    b = P.VioBatch(st.cfg, 1)
    mirror, out, worst = PR.TrackMirror(st.cfg.window_size, st.cfg.depth_min), [], [0.0]
    cap = BC.tracker_capacity(st.cfg)
    n_valid = 0
    for k, (stamp, ids, obs, depth, (ti, ai, gi), expect) in enumerate(PC.offers(st)):
        if len(ti):
            b.push_imu(0, ti, ai, gi)
        idb, ob = np.zeros((1, cap), np.int32), np.zeros((1, cap, 7))
        idb[0, :len(ids)], ob[0, :len(ids)] = ids, obs
        b.process_obs_batch([len(ids)], idb, ob, depth[None], [stamp])
        status = b.status(0)
        assert bool(status.processed) == expect, (name, k)
        if status.processed:
            mirror.frame(ids, obs, b.landmarks_ex(0), status.marginalization_flag, depth)
        pub = b.publish()
        check_live(b, 0, pub, mirror, worst, (name, k))
        n_valid += int(pub["counts"][0, 3])
        out.append(pub)
    b.close()
    print("%s: %d offers, %d keyframes, largest |dp| / bound %.3f" % (name, len(out), n_valid, worst[0]))
    assert n_valid >= 3                       # (starved, the shortest stream, has four MARGIN_OLD frames after its initialisation)
    _solo[name] = out
    return out


@pytest.mark.parametrize("name", PC.STREAMS)
def test_live_handle_equals_the_definition_after_every_frame(P, name):
    run_solo(P, name)


def test_batch_rows_equal_the_solo_runs_and_an_idle_slot_is_empty(P):
    """S = 4: short_tracks from step 0, reappear from step 2, thin from step 5 (one configuration), slot 3 never fed"""
    names, first = ("short_tracks", "reappear", "thin"), (0, 2, 5)
    streams = [PC.build(n, P) for n in names]
    solo = [run_solo(P, n) for n in names]
    cfg = streams[0].cfg
    b = P.VioBatch(cfg, 4)
    cap, H, Wd = BC.tracker_capacity(cfg), cfg.height, cfg.width
    fr = [s.frames() for s in streams]
    compared = 0
    for step in range(max(f0 + len(f) for f0, f in zip(first, fr))):
        n_obs, ids, obs = np.full(4, -1, np.int32), np.zeros((4, cap), np.int32), np.zeros((4, cap, 7))
        depth, stamps = np.zeros((4, H, Wd), np.uint16), np.zeros(4)
        live = []
        for s in range(3):
            k = step - first[s]
            if not 0 <= k < len(fr[s]):
                continue
            stamp, i, o, d, (ti, ai, gi) = fr[s][k]
            if len(ti):
                b.push_imu(s, ti, ai, gi)
            n_obs[s], ids[s, :len(i)], obs[s, :len(i)], depth[s], stamps[s] = len(i), i, o, d, stamp
            live.append((s, k))
        b.process_obs_batch(n_obs, ids, obs, depth, stamps)
        pub = b.publish()
        assert not pub["counts"][3].any() and not pub["kf_pose"][3].any() and not pub["kf_points"][3].any()
        for s, k in live:
            ref = solo[s][k]
            assert np.array_equal(pub["counts"][s], ref["counts"][0]), (step, s)
            for key in ("kf_pose", "cloud", "margin", "kf_points"):
                assert same_bits(pub[key][s], ref[key][0]), (step, s, key)
            compared += 1
        for s in range(3):
            if step < first[s]:
                assert not pub["counts"][s].any(), (step, s)
    b.close()
    assert compared == sum(len(f) for f in fr)


def _drive(P, st, upto, after=None):
    b = P.VioBatch(st.cfg, 1)
    for k, (stamp, ids, obs, depth, (ti, ai, gi)) in enumerate(st.frames()[:upto]):
        if len(ti):
            b.push_imu(0, ti, ai, gi)
        b.process_obs(0, ids, obs, depth, stamp)
        if after is not None:
            after(b, k)
    return b


def test_hbm_destination_equals_the_host_destination_and_null_lists_only_count(P):
    st = PC.build("short_tracks", P)
    seen = [0]

    def after(b, k):
        host = b.publish(fill=-7.0)
        dev = b.publish(on_device=True, fill=-7.0)
        cap = b.capacity()["landmarks"]
        assert np.array_equal(dev["counts"], host["counts"]), k
        assert same_bits(dev["kf_pose"].download(0, (1, 8), np.float64), host["kf_pose"]), k
        for key, w in (("cloud", 3), ("margin", 3), ("kf_points", 8)):
            assert same_bits(dev[key].download(0, (1, cap, w), np.float64), host[key]), (k, key)
        # the fill survives where nothing is published
        n = host["counts"][0]
        assert (host["cloud"][0, n[0]:] == -7.0).all() and (host["kf_points"][0, n[2]:] == -7.0).all()
        assert n[3] == 1 or (host["kf_pose"] == -7.0).all()
        for lists in ((False, False, False), (True, False, False), (False, False, True)):
            part = b.publish(lists=lists, cap=3)
            assert np.array_equal(part["counts"], host["counts"]), (k, lists)
            for key, on in zip(("cloud", "margin", "kf_points"), lists):
                assert (part[key] is None) == (not on)
                if on:
                    assert same_bits(part[key][0, :min(3, n[0 if key == "cloud" else 2])], host[key][0, :min(3, n[0 if key == "cloud" else 2])])
        zero = b.publish(cap=0)
        assert np.array_equal(zero["counts"], host["counts"]) and zero["cloud"].shape == (1, 0, 3)
        seen[0] += int(n[3])
        for d in (dev["kf_pose"], dev["cloud"], dev["margin"], dev["kf_points"]):
            d.free()
    _drive(P, st, 14, after).close()
    assert seen[0] >= 5


def test_publication_writer_files_hold_what_publish_returns(P, tmp_path):
    """dataio.PublicationWriter (tools/replay.py --keyframes-out / --cloud-out) on a live handle: one file per published keyframe, the last clouds"""
    import importlib
    io = importlib.import_module("vins-rgbd-fast_amd.dataio")
    pw = io.PublicationWriter(str(tmp_path / "kf"), str(tmp_path / "clouds.npz"))
    want = []

    def after(b, k):
        pw.poll(b, [0])
        want.append(b.publish())
    _drive(P, PC.build("short_tracks", P), 14, after).close()
    pw.close()
    valid = [w for w in want if w["counts"][0, 3]]
    assert pw.n_keyframes == len(valid) >= 5 and len(os.listdir(str(tmp_path / "kf"))) == len(valid)
    for w in valid:
        z = np.load(str(tmp_path / "kf" / ("kf_0_%d.npz" % int(round(w["kf_pose"][0, 0] * 1e9)))))
        assert same_bits(z["pose"], w["kf_pose"][0]) and same_bits(z["points"], w["kf_points"][0, :w["counts"][0, 2]])
    z, n = np.load(str(tmp_path / "clouds.npz")), want[-1]["counts"][0]
    assert same_bits(z["cloud_0"], want[-1]["cloud"][0, :n[0]]) and same_bits(z["margin_0"], want[-1]["margin"][0, :n[1]]) and n[0] > 20


def test_replay_writes_keyframes_and_clouds_of_every_slot(P, tmp_path):
    """dataio.replay / replay_many with publish = a PublicationWriter (tools/replay.py --keyframes-out DIR --cloud-out FILE) on written recordings:
    the files of every slot hold what publish() returned after the frame"""
    import importlib
    io = importlib.import_module("vins-rgbd-fast_amd.dataio")
    cfg = P.canonical_config()
    sc = vio_ct.synth_like(cfg)
    syn, n, recs = P.Synth(sc), 36, []
    stamps = vio_ct.frame_times(sc, n)
    for seq in (4, 5):
        frames = [syn.render_host(seq, float(t)) for t in stamps]
        ti, ai, gi = syn.imu(seq, int(n / sc.cam_rate * sc.imu_rate) + 64)
        io.write_recording(str(tmp_path / ("rec%d" % seq)), stamps, [f[0] for f in frames], [f[1] for f in frames], ti, ai, gi)
        recs.append(io.RgbdImuDirectory(str(tmp_path / ("rec%d" % seq))))
    for name, slots in (("one", 1), ("two", 2)):
        b = P.VioBatch(cfg, slots)
        pw = io.PublicationWriter(str(tmp_path / name), str(tmp_path / (name + ".npz")))
        want = {}

        def grab(*a):
            st = a[-1]
            if st.processed:
                want[(a[0] if slots == 2 else 0, len(want))] = b.publish()
        if slots == 1:
            io.replay(b, recs[0], publish=pw, on_frame=grab)
        else:
            io.replay_many(b, recs, publish=pw, on_frame=grab)
        pw.close()
        n_valid, last = 0, {}
        for (s, _), w in want.items():
            last[s] = w
            if w["counts"][s, 3]:
                z = np.load(str(tmp_path / name / ("kf_%d_%d.npz" % (s, int(round(w["kf_pose"][s, 0] * 1e9))))))
                assert same_bits(z["pose"], w["kf_pose"][s]) and same_bits(z["points"], w["kf_points"][s, :w["counts"][s, 2]])
                n_valid += 1
        assert pw.n_keyframes == n_valid >= 1 and len(os.listdir(str(tmp_path / name))) == n_valid, (pw.n_keyframes, n_valid)
        z = np.load(str(tmp_path / (name + ".npz")))
        for s, w in last.items():
            assert same_bits(z["cloud_%d" % s], w["cloud"][s, :w["counts"][s, 0]]) and w["counts"][s, 0] > 20
            assert same_bits(z["margin_%d" % s], w["margin"][s, :w["counts"][s, 1]])
        b.close()


def test_publishing_leaves_the_handle_as_it_was(P):
    """a handle polled twice after every frame (identical answers) ends with the window, prior and status bytes of one never polled"""
    st = PC.build("thin", P)

    def after(b, k):
        a1, a2 = b.publish(), b.publish()
        assert np.array_equal(a1["counts"], a2["counts"])
        assert all(same_bits(a1[key], a2[key]) for key in ("kf_pose", "cloud", "margin", "kf_points")), k
    polled, quiet = _drive(P, st, None, after), _drive(P, st, None)
    assert same_bits(polled.window(0), quiet.window(0))
    sp, sq = status_dict(polled.status(0)), status_dict(quiet.status(0))
    assert sp == sq, (sp, sq)
    pp, pq = polled.prior(0), quiet.prior(0)
    assert pp is not None and all(np.array_equal(x, y) for x, y in zip(pp, pq))
    assert np.array_equal(polled.save([0])[0], quiet.save([0])[0])
    polled.close(); quiet.close()


def test_image_fed_handle_with_tracker_lag_and_the_split_marginalisation(P, monkeypatch):
    """the configuration of tests/test_gpu_marg_split.py (S = 3, 640 x 480, window 4, tracker lag 1, VIO_MARG_SPLIT = 1): be_marg's second half
    runs beside the next frame's ingest; after every vio_feed pose rows, counts, order, ids and points agree with the getters"""
    import test_gpu_marg_split as MS
    cfg = MS._cfg(P)
    seqs, times = MS._canonical_plan(P, cfg)
    r = MS.Run(P, monkeypatch, cfg, seqs, times, 1)
    worst, valid = [0.0], np.zeros(3, int)
    for f in range(len(times)):
        r.feed(f)
        pub = r.b.publish()
        for s in range(3):
            check_live(r.b, s, pub, None, worst, (f, s), obs=False)
        valid += pub["counts"][:, 3]
    split = r.b.marg_split_stats(per_seq=True)
    r.b.close()
    print("image-fed: keyframes per sequence %s, split marginalisations %s, largest |dp| / bound %.3f" % (valid, split, worst[0]))
    assert (split[1:] >= 6).all() and (valid[1:] >= 6).all(), (split, valid)


# ------------------------------------------------------------------------------------------------------------- the chain, the C++ mirror
def _q2R(q):
    return PR.quat_to_R(q)


def test_loop_chain_from_a_published_keyframe(P):
    """The scenario of test_gpu_posegraph.test_loop_verification_feeds_the_relocalisation_of_a_live_estimator, same sizes, on two handles fed
    alike: one gets the keyframe of window frame W-2 built by hand from remembered feature maps and the getters, the other the one
    KeyFrame.from_publication builds from publish() alone.  Both next solves carry the same relocalisation factors and vio_get_relo bytes."""
    import importlib
    import test_oracle_posegraph_cpu as O
    PG = importlib.import_module("vins-rgbd-fast_amd.posegraph")
    cfg = P.canonical_config()
    sc = vio_ct.synth_like(cfg)
    syn = P.Synth(sc)
    pat = O.pattern()
    W = cfg.window_size
    seq, n_frames, f_set, i_local, back = 3, 40, 36, W - 2, 2
    times = vio_ct.frame_times(sc, n_frames)
    ti, ai, gi = syn.imu(seq, int(n_frames / sc.cam_rate * sc.imu_rate) + 64)
    hand, publ = P.VioBatch(cfg, 1), P.VioBatch(cfg, 1)
    ric, tic = np.array(list(cfg.ric)).reshape(3, 3), np.array(list(cfg.tic))
    maps, imgs, k, out = {}, {}, 0, {}
    for f in range(f_set + 2):
        tf = float(times[f])
        k2 = vio_ct.imu_until(ti, k, tf, sc.imu_rate)
        g, d = syn.render_host(seq, tf)
        for b in (hand, publ):
            b.push_imu(0, ti[k:k2], ai[k:k2], gi[k:k2])
            b.feed(g[None], d[None], [tf])
        k = k2
        maps[round(tf, 6)] = hand.packaged(0)
        imgs[round(tf, 6)] = g
        if f == f_set:
            w = hand.window(0)
            stamp_i, stamp_k = float(w[i_local, 16]), float(w[i_local - back, 16])
            ids_i, obs_i = maps[round(stamp_i, 6)]
            at = {int(fid): j for j, fid in enumerate(ids_i)}
            rows = []
            for r in hand.landmarks_ex(0):          # pubKeyframe's rule, in list order
                s0, n = int(r[1]), int(r[2])
                if not (s0 < W - 2 and s0 + n - 1 >= W - 2 and int(r[5]) == 1):
                    continue
                j = at[int(r[0])]
                dep = r[3] if r[10] == 0 else r[10]
                p3 = _q2R(w[s0, 3:7]) @ (ric @ (dep * r[7:10]) + tic) + w[s0, :3]
                rows.append(np.concatenate([p3, obs_i[j, 0:2], obs_i[j, 3:5], [r[0]]]))
            rows = np.array(rows)
            assert hand.status(0).marginalization_flag == 0 and len(rows) > 60
            cur_hand = PG.KeyFrame(cfg, pat, stamp_i, 7, w[i_local, :3], _q2R(w[i_local, 3:7]), imgs[round(stamp_i, 6)], rows[:, 0:3], rows[:, 5:7],
                                   rows[:, 3:5], rows[:, 7])
            pub = publ.publish()
            assert pub["counts"][0, 3] == 1 and pub["counts"][0, 2] == len(rows)
            cur_publ = PG.KeyFrame.from_publication(cfg, pat, 7, pub["kf_pose"][0], pub["kf_points"][0, :pub["counts"][0, 2]],
                                                    imgs[round(float(pub["kf_pose"][0, 0]), 6)])
            assert cur_publ.time_stamp == stamp_i
            assert np.array_equal(cur_publ.point_id, cur_hand.point_id) and np.array_equal(cur_publ.point_2d_uv, cur_hand.point_2d_uv)
            assert np.array_equal(cur_publ.point_2d_norm, cur_hand.point_2d_norm)
            assert np.abs(cur_publ.point_3d - cur_hand.point_3d).max() < 1e-5
            p_gt_k, R_gt_k, _ = syn.pose(seq, stamp_k)
            old = PG.KeyFrame(cfg, pat, stamp_k, 3, p_gt_k, R_gt_k, imgs[round(stamp_k, 6)], np.zeros((0, 3)), np.zeros((0, 2)), np.zeros((0, 2)), np.zeros(0))
            for b, cur in ((hand, cur_hand), (publ, cur_publ)):
                assert cur.findConnection(old, ric, tic)
                assert len(cur.match_points) > PG.MIN_LOOP_NUM
                b.set_relo_frame(0, stamp_i, cur.index, cur.match_points, old.T_w_i, old.R_w_i)
            assert np.array_equal(cur_hand.match_points, cur_publ.match_points)
        if f == f_set + 1:
            for key, b in (("hand", hand), ("publ", publ)):
                o = np.zeros(30)
                b._chk(b.L.vio_get_relo(b.h, 0, o.ctypes.data), "vio_get_relo")
                out[key] = o
    hand.close(); publ.close()
    assert out["hand"][29] >= PG.MIN_LOOP_NUM and out["hand"][29] == out["publ"][29]
    assert same_bits(out["hand"], out["publ"])


def test_cpp_mirror_keyframe_and_margin_cloud_equal_publish(P, tmp_path):
    exe = str(tmp_path / "publish_demo")
    pk = os.path.join(ROOT, "vins-rgbd-fast_amd")
    r = subprocess.run(["g++", "-std=c++11", "-O1", "-Wall", "-I" + os.path.join(ROOT, "include"), os.path.join(ROOT, "examples", "publish_demo.cpp"),
                        "-L" + pk, "-lvio_hip", "-Wl,-rpath," + pk, "-o", exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    out = subprocess.run([exe, "2", "30"], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stderr
    rows = np.array([[float(x) for x in line.split()] for line in out.stdout.strip().splitlines()])
    assert len(rows) >= 20 and (rows[:, 5] == 1).all(), rows
    assert (rows[:, 1] == 1).sum() >= 5 and rows[rows[:, 1] == 1, 2].min() > 20 and rows[:, 4].max() > 20, rows
