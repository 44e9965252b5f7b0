"""IMU-rate odometry for the whole batch (vio_get_latest_odometry_all / vio_get_imu_rate_odometry): what can be checked without a GPU.
The library's exports and argument checks, and the numpy definition the GPU tests use (imu_rate_ref.py) pinned against the oracle's
Estimator::latestOdometry, sample by sample, in both modes of reference_quirks bit 0."""
import ctypes as C

import numpy as np
import pytest

import imu_rate_ref
import vio_ct

VIO_EINVAL = -1


def test_the_batched_getters_are_exported(P):
    L = P.lib()
    for name in ("vio_get_latest_odometry_all", "vio_get_imu_rate_odometry"):
        assert hasattr(L, name), name
    assert hasattr(P.VioBatch, "latest_odometry_all") and hasattr(P.VioBatch, "imu_rate_odometry")


def test_a_null_handle_is_refused(P):
    L = P.lib()
    out, n = np.zeros(11), np.zeros(1, np.int32)
    assert L.vio_get_latest_odometry_all(None, out.ctypes.data, 0) == VIO_EINVAL
    assert L.vio_get_imu_rate_odometry(None, None, 1, n.ctypes.data, out.ctypes.data, 0) == VIO_EINVAL
    assert L.vio_get_imu_rate_odometry(None, None, 0, n.ctypes.data, None, 0) == VIO_EINVAL


@pytest.mark.parametrize("quirk", [0, 1])
def test_the_numpy_definition_follows_the_oracle_sample_by_sample(P, quirk):
    """OraclePipeline to solver_flag == 1, then 20 samples pushed one at a time: after the k-th push ovio_latest_odometry is row k of the
    definition computed ONCE over all of them (time 1e-12, the rest 1e-6: the bars of test_gpu_parity2's replay)."""
    cfg = P.canonical_config(reference_quirks=quirk)
    sc = vio_ct.synth_like(cfg)
    seq, n_max, n_more = 14, 30, 20
    syn = P.Synth(sc)
    ti, ai, gi = syn.imu(seq, int(n_max / sc.cam_rate * sc.imu_rate) + 64)
    o = vio_ct.OraclePipeline(cfg)
    k = 0
    for tf in vio_ct.frame_times(sc, n_max):
        k2 = vio_ct.imu_until(ti, k, tf, sc.imu_rate)
        o.push_imu(ti[k:k2], ai[k:k2], gi[k:k2]); k = k2
        g, d = syn.render_host(seq, float(tf))
        o.feed(g, d, tf)
        if o.status()["solver_flag"] == 1:
            break
    assert o.status()["solver_flag"] == 1
    w = o.window()[cfg.window_size]
    gvec = np.array([0, 0, cfg.g_norm])
    rows, state = imu_rate_ref.imu_rate_rows(w, o.status()["td"], gvec, ti[:k + n_more], ai[:k + n_more], gi[:k + n_more], k, quirk)
    n0 = int((ti[:k] > w[16] + o.status()["td"]).sum())    # samples beyond the frame that were pushed with it
    assert n0 >= 1 and len(rows) == n0 + n_more
    def close(a, b):
        assert abs(a[0] - b[0]) < 1e-12 and np.abs(a[1:] - b[1:]).max() < 1e-6, (a - b)
    close(o.latest_odometry(), rows[n0 - 1])
    for j in range(n_more):
        o.push_imu(ti[k + j:k + j + 1], ai[k + j:k + j + 1], gi[k + j:k + j + 1])
        close(o.latest_odometry(), rows[n0 + j])
    assert np.linalg.norm(rows[-1, 1:4] - state[1:4]) > 1e-3                         # the pose really moved with the IMU
    if quirk:   # the switch changes the rows
        r0, _ = imu_rate_ref.imu_rate_rows(w, o.status()["td"], gvec, ti[:k + n_more], ai[:k + n_more], gi[:k + n_more], k, 0)
        assert np.linalg.norm(rows[-1, 1:4] - r0[-1, 1:4]) > 1e-9
