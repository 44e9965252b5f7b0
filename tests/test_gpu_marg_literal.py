"""The literal marginalisation (vio_config.marg_exact = 1 / 2) stage by stage against its definition, through vio_stage_marg_literal
(be_stage_marg_literal_kernel calls marg_exact_finish / marg_literal_prior / marg_certificate of be_kernels.hip directly, as be_marg_exact_kernel
does: one workgroup of 256 or 512 threads, the same dynamic LDS).  The references, the inputs and every bound are those of tests/marg_ref.py
(its docstring derives them; tests/test_marg_ref_cpu.py shows a float64 numpy evaluation inside them on the same inputs).

  part 0  marg_exact_finish: A_mm^+, A_r, b_r at m = 6, 15 .. 32 (mpmath), on both sides of the LDS / HBM switch of the first eigen-decomposition
          (forced at 40, and where a handle puts it), 128 / 129, 215 and 495; well-conditioned, graded, dropped landmarks, an exact null
          direction, an asymmetric A, and landmarks at the 1e-8 cut.  Cl has ldc > m + n with NaN in the padding.
  part 1  marg_literal_prior: n = 1 .. 136 on both sides of the switch, four kinds of spectrum, the strictness of `ev > 1e-8`, NaN input.
  part 2  marg_certificate: soundness and completeness over a sweep of lambda_min(A_mm), the bound's value, the refusals.
  pipeline  what the three modes must share exactly (everything up to the first marginalising frame), how far mode 2's first prior may lie from
          mode 0's, per-frame sanity of modes 1 and 2, that the streams reach m = 6, m = 15, both sides of MXL and n = 136, and that mode 2's
          count of uncertified frames does not depend on the number of marginalisation threads.  (Pinv, the certificate's input, lives in LDS only:
          the count cannot be recomputed from a snapshot, so the second of the two checks the issue offers is the one made.)

Why a diagonal input is exact in both eigen-solvers (the strictness cases rely on it).  sym_eig_tridiag_mt (be_linalg.h): every row i has
sc = sum |d[k]| == 0.0, so the `if (sc == 0.0)` branch only copies (e[i] = d[i - 1] = 0, d[i] = 0.0) and the accumulation skips every step
(`if (h != 0.0)` with h = d[i + 1] = 0); the diagonal comes back through `d[j] = V[(n - 1) * ld + j]`.  tridiag_ql_wave: every e[l] is 0, so
`m == l`, no sweep runs, f stays 0.0 and `d[l] = d[l] + f` returns d[l].  sym_eig_hbm has the same three places (`if (sc == 0.0)`,
`if (h != 0.0)`, `if (m > l)`).  So eigenvalue k IS a_kk and eigenvector k is e_k, and `1e-8 > 1e-8` is decided on the input's own bits.  With a
full pose block beside the two landmarks the eigenvalues of the decoupled landmarks still pass through `d[i] -= h` ... `d[l] + f` (the QL
shifts of the rows before them), which costs their last bits: that case (strict_general) uses 0.9e-8 / 1.1e-8.
Both QL loops are capped (`iter < 60`, be_linalg.h tridiag_ql_wave and sym_eig_hbm), and `tst1` never becomes NaN (fmax), so NaN input ends."""
import ctypes as C
import functools

import numpy as np
import pytest

import backend_cases as BC
import marg_ref as M
import test_gpu_marg_lds as ML

pytestmark = pytest.mark.gpu

L = np.longdouble
VIO_EINVAL = -1
NPRIOR_MAX = 136
_worst = {}


def _note(fam, ratios):
    for k, v in ratios.items():
        if k != "rows":
            _worst[(fam, k)] = max(_worst.get((fam, k), 0.0), float(v))


def _ptr(a):
    return None if a is None else a.ctypes.data


def _call(P, part, md, F0, n, ldc, nt, mxl, A, b=None, Cl=None, Hll=None, gl=None, pinv_direct=1, second_new=0):
    Lb = P.lib()
    Lb.vio_stage_marg_literal.argtypes = [C.c_int] * 9 + [C.c_void_p] * 14
    Lb.vio_stage_marg_literal.restype = C.c_int
    m = md + F0
    arrs = [None if x is None else np.ascontiguousarray(x, np.float64) for x in (A, b, Cl, Hll, gl)]
    o = dict(X=np.zeros((m, m)), Ar=np.zeros((n, n)), br=np.zeros(n), J=np.zeros((n, n)), rf=np.zeros(n), H=np.zeros((n, n)), r=np.zeros(n),
             scal=np.zeros(2), info=np.zeros(8, np.int32))
    rc = Lb.vio_stage_marg_literal(part, md, F0, n, ldc, nt, mxl, pinv_direct, second_new, *[_ptr(x) for x in arrs],
                                   *[_ptr(o[k]) for k in ("X", "Ar", "br", "J", "rf", "H", "r", "scal", "info")])
    o["rc"] = rc
    return o


def _stage(P, part, md, F0, n, ldc, nt, mxl, A, **kw):
    """the call with what holds always: return code 0, guard words intact, and for part 0 dbg[0] = 0, dbg[2] = second_new, dbg[4] = m"""
    o = _call(P, part, md, F0, n, ldc, nt, mxl, A, **kw)
    assert o["rc"] == 0, (o["rc"], part, md, F0, n, nt, mxl)
    assert o["info"][1] == 1, ("guard words", part, md, F0, n, nt, mxl)
    assert o["info"][0] == (mxl if mxl else o["info"][0]) and 1 <= o["info"][0] <= 128
    if part == 0:
        assert tuple(o["info"][3:6]) == (0, kw.get("second_new", 0), md + F0), o["info"]
    else:
        assert tuple(o["info"][3:6]) == (-1, -1, -1), o["info"]      # only marg_exact_finish writes them (mode 2: marg_body itself)
    return o


@functools.lru_cache(maxsize=None)
def _mxl(P):
    """the MXL a handle chooses, as the harness reports it"""
    A, b = np.eye(1), np.ones(1)
    return int(_stage(P, 1, 15, 0, 1, 16, 256, 0, A, b=b)["info"][0])


def _size(P, label):
    Mx = _mxl(P)
    return {"M": Mx, "M+1": Mx + 1}.get(label, label)


# ------------------------------------------------------------------------------------------------------------------------------ part 0
def _run0(P, s, nt, mxl):
    o = _stage(P, 0, s.md, s.F0, s.n, s.ldc, nt, mxl, s.A, b=s.b, Cl=s.Cl if s.F0 else None, Hll=s.d if s.F0 else None,
               gl=s.gl if s.F0 else None, second_new=1 if s.md == 6 else 0)
    for k in ("X", "Ar", "br", "J", "rf", "H", "r"):
        assert np.all(np.isfinite(o[k])), (k, "not finite (a read of Cl's NaN padding would show here)")
    return o


def _check0(P, kind, md, F0, n, nt, mxl):
    s = M.part0_case(kind, md, F0, n)
    ref = M.part0_ref(kind, md, F0, n)
    assert s.ldc > s.mq and (F0 == 0 or np.all(np.isnan(s.Cl[:, s.mq:])))
    o = _run0(P, s, nt, mxl)
    what = (kind, md, F0, n, nt, mxl)
    ratios = M.check_part0(ref, o["X"], o["Ar"], o["br"])
    print("part0", what, {k: "%.4f" % v for k, v in ratios.items()})
    _note("p0 " + kind, ratios)
    assert all(v <= 1.0 for v in ratios.values()), (what, ratios)
    if kind.startswith("drop") or kind.startswith("strict"):
        gone = np.where(s.d <= M.CUT)[0] + md
        assert len(gone) == ref.n_dropped and not np.any(o["X"][gone]) and not np.any(o["X"][:, gone]), what      # dropped: exactly nothing left
    if kind == "strict":
        assert o["X"][ref.i_hi, ref.i_hi] == 2.0 ** 26, (what, o["X"][ref.i_hi, ref.i_hi])                        # 2^-26 > 1e-8 is kept, exactly
    if kind.startswith("strict"):
        assert o["X"][ref.i_hi, ref.i_hi] > 0.0 and np.count_nonzero(o["X"][ref.i_hi]) == 1, what
    if kind == "dropall":
        s0, r0 = M.part0_case("well", md, 0, n), M.part0_ref("well", md, 0, n)
        o0 = _run0(P, s0, nt, mxl)
        assert M.norm2(o["X"][:md, :md] - o0["X"]) <= ref.bx + r0.bx, what
    # the second half as part 0 runs it, on the A_r and b_r it computed itself: every direction kept
    r1 = M.ref1_all_kept(o["Ar"], o["br"])
    out = M.check_part1(r1, o["J"], o["rf"], o["H"], o["r"], float(o["scal"][0]))
    _note("p0 prior", out)
    assert out.pop("rows") == n and all(v <= 1.0 for v in out.values()), (what, out)
    return o


P0_SIZES = [(6, 0, 0), (15, 0, 0), (15, 1, 0), (15, 2, 0), (15, 16, 0), (15, 17, 0), (15, 25, 40), (15, 26, 40), (15, "M", 0), (15, "M+1", 0),
            (15, 128 - 15, 0), (15, 129 - 15, 0), (15, 215 - 15, 0)]


@pytest.mark.parametrize("nt", [256, 512])
@pytest.mark.parametrize("md,F0,mxl", P0_SIZES)
def test_part0_against_the_definition(P, md, F0, mxl, nt):
    if isinstance(F0, str):
        F0 = _size(P, F0) - md
    for kind in M.part0_kinds(md, F0):
        _check0(P, kind, md, F0, M.P0_N, nt, mxl)


def test_part0_at_the_largest_block(P):
    for kind in ("well", "graded", "drop3"):
        _check0(P, kind, 15, 480, 76, 512, 0)


def test_part0_forced_switch_is_taken_where_it_is_forced(P):
    """m = 40 and 41 with mxl = 40 are compared with the same kind of reference above; here: m = 41 run LDS-resident (mxl = 41) and on HBM
    (mxl = 40) both satisfy the bounds but need not be the same bits, and the effective mxl is reported as given"""
    s = M.part0_case("well", 15, 26, M.P0_N)
    a, b = _run0(P, s, 512, 41), _run0(P, s, 512, 40)
    assert a["info"][0] == 41 and b["info"][0] == 40
    ref = M.part0_ref("well", 15, 26, M.P0_N)
    assert M.norm2(a["X"] - b["X"]) <= 2 * ref.bx
    assert 16 <= _mxl(P) <= 128


# ------------------------------------------------------------------------------------------------------------------------------ part 1
def _run1(P, A, b, nt, mxl):
    n = A.shape[0]
    return _stage(P, 1, 15, 0, n, n + 15, nt, mxl, A, b=b)


def _check1(P, kind, n, nt, mxl):
    A, b, ref = M.part1_case(kind, n)
    o = _run1(P, A, b, nt, mxl)
    out = M.check_part1(ref, o["J"], o["rf"], o["H"], o["r"], float(o["scal"][0]))
    print("part1", (kind, n, nt, mxl), {k: ("%.4f" % v if k != "rows" else v) for k, v in out.items()})
    _note("p1 " + kind, out)
    assert out.pop("rows") == ref.n_kept, (kind, n, nt, mxl, ref.n_kept)
    assert all(v <= 1.0 for v in out.values()), (kind, n, nt, mxl, out)


@pytest.mark.parametrize("n,mxl", [(1, 0), (2, 0), (22, 0), (22, 16), (76, 0), ("M", 0), ("M+1", 0), (128, 0), (129, 0), (136, 0)])
def test_part1_against_the_definition(P, n, mxl):
    n = _size(P, n)
    for nt in (256, 512):
        for kind in M.PART1_KINDS:
            _check1(P, kind, n, nt, mxl)


@pytest.mark.parametrize("n,mxl", [(22, 0), (22, 16), (136, 0)])
def test_part1_cut_is_strict(P, n, mxl):
    """diag(1e-8, 2^-26, 1, ...): both solvers return a diagonal input exactly (module docstring), so 1e-8, which is not > 1e-8, leaves a zero row of
    J and a zero in rf, and 2^-26 is kept with its exact square root"""
    A, b = M.strict_diagonal(n)
    for nt in (256, 512):
        o = _run1(P, A, b, nt, mxl)
        assert not np.any(o["J"][0]) and o["rf"][0] == 0.0, (n, nt, mxl, o["rf"][0])
        assert o["J"][1, 1] == 2.0 ** -13 and np.count_nonzero(o["J"][1]) == 1 and o["rf"][1] == 2.0 * 2.0 ** 13, (n, nt, mxl)
        assert np.count_nonzero(np.any(o["J"] != 0, axis=1)) == n - 1
        assert o["H"][0, 0] == 0.0 and o["r"][0] == 0.0 and o["H"][1, 1] == 2.0 ** -26 and o["r"][1] == 2.0


@pytest.mark.parametrize("mxl", [0, 16])
def test_part1_returns_on_non_finite_input(P, mxl):
    """a contract check: NaN in A_r ends (both QL loops are capped at 60 sweeps per eigenvalue) and writes nothing outside its arrays"""
    A, b, _ = M.part1_case("kept", 22)
    A = A.copy()
    A[3, 5] = A[5, 3] = np.nan
    _run1(P, A, b, 512, mxl)


# ------------------------------------------------------------------------------------------------------------------------------ part 2
def _cert(P, c, nt, **kw):
    Cl, dinv = kw.pop("Cl", c.Cl), kw.pop("dinv", c.dinv)
    Pinv = kw.pop("Pinv", c.Pinv)
    o = _stage(P, 2, c.md, c.F0, 22, c.ldc, nt, 0, Pinv, Cl=Cl if c.F0 else None, Hll=dinv if c.F0 else None, **kw)
    return bool(o["info"][2]), float(o["scal"][1])


@pytest.mark.parametrize("md,F0", M.CERT_SIZES)
def test_certificate_is_sound_complete_and_its_bound_right(P, md, F0):
    seen = set()
    for lam in M.CERT_SWEEP:
        c = M.cert_case(md, F0, lam)
        for nt in (256, 512):
            ok, bound = _cert(P, c, nt)
            assert not ok or c.lam_min > 1e-7, (md, F0, lam, nt)                            # soundness, no exceptions
            if c.inv_bound >= 2e-7:
                assert ok, (md, F0, lam, nt, c.inv_bound)
            if c.inv_bound <= 0.5e-7:
                assert not ok, (md, F0, lam, nt, c.inv_bound)
            rel = abs(bound - float(c.bound)) / float(c.bound) / (M.C * (F0 + md) * M.EPS)
            _note("p2", {"bound": rel})
            assert rel <= 1.0, (md, F0, lam, nt, bound, float(c.bound))
            seen.add(ok)
    print("part2", (md, F0), "worst rel", _worst[("p2", "bound")])
    assert seen == {True, False}


def test_certificate_refuses(P):
    c = M.cert_case(15, 17, 1e-3)
    for nt in (256, 512):
        assert _cert(P, c, nt)[0]
        assert not _cert(P, c, nt, pinv_direct=0)[0]
        for v in (0.0, -1.0):
            dinv = c.dinv.copy()
            dinv[5] = v
            assert not _cert(P, c, nt, dinv=dinv)[0], v
        Pn = c.Pinv.copy()
        Pn[3, 4] = np.nan
        assert not _cert(P, c, nt, Pinv=Pn)[0]


def test_certificate_second_new_ignores_the_landmarks_and_an_empty_block_is_the_pose_block(P):
    c = M.cert_case(6, 3, 1e-3)
    for nt in (256, 512):
        ok, bound = _cert(P, c, nt, second_new=1, Cl=np.full_like(c.Cl, np.nan), dinv=np.full_like(c.dinv, np.nan))
        ref = float(M.cert_bound_ld(c.Pinv, c.Cl, c.dinv, second_new=True))
        assert ok and abs(bound - ref) <= M.C * 6 * M.EPS * ref
        e = M.cert_case(15, 0, 1e-3)
        ok, bound = _cert(P, e, nt)
        assert ok and abs(bound - float(np.sqrt((e.Pinv.astype(L) ** 2).sum()))) <= M.C * 15 * M.EPS * bound


def test_wrong_arguments_are_refused(P):
    A, b = np.eye(22), np.ones(22)
    good = dict(part=1, md=15, F0=0, n=22, ldc=40, nt=256, mxl=0)
    assert _call(P, A=A, b=b, **good)["rc"] == 0
    for bad in (dict(md=7), dict(F0=481), dict(n=NPRIOR_MAX + 1), dict(mxl=129), dict(nt=96), dict(part=3), dict(part=0, ldc=36)):
        kw = dict(good, **bad)
        n = min(kw["n"], NPRIOR_MAX + 1)
        assert _call(P, A=np.eye(15 + n), b=np.ones(15 + n), **kw)["rc"] == VIO_EINVAL, bad
    assert _call(P, A=None, b=b, **good)["rc"] == VIO_EINVAL


# ------------------------------------------------------------------------------------------------------------------------------ the pipeline
PIPE_STREAMS = dict({k: ML.STREAMS[k][0] for k in ("second_new_run", "no_anchor_in_frame_0", "f0_above_64", "f0_above_128", "slide_drops_all",
                                                   "w10_td")}, w20=BC.w20_moving)


def _pipe(P, st, mode, monkeypatch, threads=512):
    cfg = type(st.cfg).from_buffer_copy(bytes(st.cfg))
    cfg.marg_exact = mode
    for k in ML.KNOBS:
        monkeypatch.delenv(k, raising=False)
    monkeypatch.setenv("VIO_MARG_THREADS", str(threads))
    b = P.VioBatch(cfg, 1)
    Lb = P.lib()
    Lb.vio_debug_seq.argtypes = [C.c_void_p, C.c_int, C.c_void_p]
    lay = {name: (off, nbytes) for name, kind, nbytes, off in b.snapshot_layout()}
    h0 = C.sizeof(P.SnapshotHeader)
    n = 6 * cfg.window_size + 16
    out = []
    for stamp, ids, obs, depth, (ti, ai, gi) in st.frames():
        if len(ti):
            b.push_imu(0, ti, ai, gi)
        b.process_obs(0, ids, obs, depth, stamp)
        blob = b.save([0])[0]
        dbg = np.zeros(16, np.int32)
        Lb.vio_debug_seq(b.h, 0, dbg.ctypes.data)
        off, nb = lay["prior_H"]
        pr = b.prior(0) if mode == 0 else None      # (mode 0 only: which poses the prior holds is a matter of structure, the same in every mode)
        out.append(dict(status=ML._status(b, 0), window=b.window(0).copy(), lm=b.landmarks_ex(0).copy(), dbg=dbg, cert=b.marg_certificate(0),
                        present=None if pr is None else pr[3].copy(),
                        prior_H=np.frombuffer(blob[h0 + off:h0 + off + nb].tobytes(), np.float64)[:n * n].reshape(n, n).copy()))
    b.close()
    return out


@pytest.mark.parametrize("name", list(PIPE_STREAMS))
def test_pipeline_in_the_literal_modes(P, monkeypatch, name):
    st = PIPE_STREAMS[name](P)
    W = st.cfg.window_size
    n = 6 * W + 16
    runs = {mode: _pipe(P, st, mode, monkeypatch) for mode in (0, 1, 2)}
    ref = runs[0]
    first = min(k for k in range(len(ref)) if ref[k]["status"]["has_prior"])
    assert ref[-1]["status"]["solver_flag"] == 1 and first < len(ref) - 1
    # the modes differ only inside be_marg: up to and including the first marginalising frame everything a handle shows is the same bits
    for mode in (1, 2):
        for k in range(first + 1):
            a, r = runs[mode][k], ref[k]
            assert a["status"] == r["status"], (mode, k, a["status"], r["status"])
            assert np.array_equal(a["window"].view(np.uint64), r["window"].view(np.uint64)), (mode, k)
            assert np.array_equal(a["lm"].view(np.uint64), r["lm"].view(np.uint64)), (mode, k)
    # mode 2's first half is mode 0's code: its first prior is J^T J of the truncated factors of the same sym(A_r)
    H0, H2 = ref[first]["prior_H"], runs[2][first]["prior_H"]
    nH = M.norm2(H0)
    assert nH > 0 and M.norm2(H2 - H0) <= 2e-8 + 2 * M.C * n * M.EPS * nH, (M.norm2(H2 - H0), nH)
    mxl = _mxl(P)
    reach = []
    for mode in (1, 2):
        run = runs[mode]
        for k in range(first, len(run)):
            s, H = run[k]["status"], run[k]["prior_H"]
            assert np.all(np.isfinite(H)), (mode, k)
            nrm = M.norm2(H)
            assert np.abs(H - H.T).max() <= M.gamma(n) * nrm, (mode, k)
            assert np.linalg.eigvalsh(0.5 * (H + H.T))[0] >= -M.C * n * M.EPS * nrm, (mode, k)
            assert s["overflow_flags"] == 0 and s["reboot_count"] == ref[k]["status"]["reboot_count"], (mode, k, s)
            if s["solver_flag"] != 1 or run[k - 1]["status"]["solver_flag"] != 1:
                continue
            dbg = run[k]["dbg"]
            if s["marginalization_flag"] == 0:
                want = 15 + BC.anchored(run[k - 1]) if mode == 1 else 15
                assert (dbg[0], dbg[2], dbg[4]) == (0, 0, want), (mode, k, dbg[:5], want)
                if mode == 1:
                    reach.append(want)
            else:
                # MARGIN_SECOND_NEW marginalises (md = 6) only while the prior holds pose W - 1, as the reference does: mode 0's prior says whether
                # it does, as long as this run has made mode 0's keyframe decisions so far.  The solve clears dbg[4]; only a marginalisation sets it
                assert (dbg[2], dbg[4]) == (1, 6) or dbg[4] == 0, (mode, k, dbg[:5])
                same = all(run[q]["status"][f] == ref[q]["status"][f] for q in range(k + 1) for f in ("marginalization_flag", "has_prior", "solver_flag"))
                if same and ref[k - 1]["present"] is not None:
                    runs_marg = bool(ref[k - 1]["present"][W - 1])
                    assert (dbg[4] == 6) == runs_marg, (mode, k, dbg[:5], ref[k - 1]["present"])
                if mode == 1 and dbg[4] == 6:
                    assert dbg[0] == 0
                    reach.append(6)
    print("pipeline", name, "m reached in mode 1:", sorted(set(reach)), "MXL", mxl, "uncertified", runs[2][-1]["cert"])
    if name == "second_new_run":
        assert 6 in reach
    elif name == "no_anchor_in_frame_0":
        assert 15 in reach
    elif name == "f0_above_64":
        assert max(reach) <= mxl and max(reach) > 15 + 64
    elif name == "f0_above_128":
        assert max(reach) > mxl
    elif name == "w20":
        assert n == NPRIOR_MAX and n > 128 >= mxl and len([m for m in reach if m >= 15]) >= 5
    # mode 2's count of uncertified frames is a property of the frames, not of the launch: the same at 256 and 512 marginalisation threads
    c256, c512 = _pipe(P, st, 2, monkeypatch, threads=256), runs[2]
    assert [r["cert"][0] for r in c256] == [r["cert"][0] for r in c512]
    assert [r["dbg"][12] for r in c256] == [r["cert"][0] for r in c256]


def test_zz_report_worst_ratios(P):
    """(prints the worst error / bound per part and kind that DESIGN.md 5a records; run with -s)"""
    for k in sorted(_worst):
        print("worst %-22s %-6s %.4f" % (k[0], k[1], _worst[k]))
