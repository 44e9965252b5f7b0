"""The streams of pg_batch_cases.py reach the branches they are named for -- shown with the oracle's DBoW2 restatement alone (oracle/bow.cpp
through bow_util.OracleVoc), no GPU.  test_gpu_pg_batch.py runs the same streams through the device's batched database."""
import numpy as np
import pytest

import bow_util
import pg_batch_cases as bc


@pytest.fixture(scope="module")
def recs():
    return [bc.replay_oracle(s) for s in bc.streams()]


def _by_frame(rec):
    return {r["frame"]: r for r in rec if r is not None}


def test_revisiting_sequence_finds_loops_and_short_one_none(recs):
    loops = [r for r in recs[bc.REVISIT] if r is not None and r["loop"] != -1]
    assert len(loops) >= 5 and all(r["frame"] > 50 for r in loops)
    # the candidate is an old keyframe of the revisited place, never the newest entry
    assert all(r["loop"] < r["frame"] - 50 for r in loops)
    short = [r for r in recs[bc.SHORT] if r is not None]
    assert len(short) == 50 and max(r["frame"] for r in short) == 49 and all(r["loop"] == -1 for r in short)


def test_sparse_sequence_lags_and_mixes_modes(recs):
    stream, rec = bc.streams()[bc.SPARSE], recs[bc.SPARSE]
    modes = [m for m, _ in stream]
    assert modes.count(0) > 10 and modes.count(2) > 5 and modes.count(1) > 40
    lag = [t - r["frame"] for t, r in enumerate(rec) if r is not None]
    assert lag[0] == 0 and lag[-1] > 10 and all(b >= a for a, b in zip(lag, lag[1:]))
    # a mode-2 keyframe enters the database all the same: later queries can return it
    added = {r["frame"] for r in rec if r is not None and r["mode"] == 2}
    assert any(int(i) in added for r in rec if r is not None for i in r["ids"])
    assert any(r is not None and r["loop"] != -1 for r in rec)


def test_equal_scores_and_result_counts(recs):
    f = _by_frame(recs[bc.TIES])
    r = f[52]
    ids = [int(i) for i in r["ids"]]
    assert sorted(ids) == [0, 1, 51] and ids.index(1) == ids.index(0) + 1          # equal scores: the smaller entry id first
    assert r["scores"][ids.index(0)] == r["scores"][ids.index(1)] > 0.015
    assert len(f[0]["ids"]) == 0                                   # empty database
    assert len(f[50]["ids"]) == 1 and f[50]["ids"][0] == 49        # cut-off 0: only the newest entry is eligible
    assert len(f[51]["ids"]) == 2
    counts = {len(r["ids"]) for rec in recs for r in rec if r is not None and r["mode"] == 1}
    assert {0, 1, 3, 4} <= counts


@pytest.mark.parametrize("seq", [bc.REVISIT, bc.SHORT])
def test_frame_49_queries_every_entry(recs, seq):
    """frame_index 49: max_id = -1, every entry is eligible.  The results name an entry that is neither the newest (48) nor below max_id
    under any other reading (no id is below -1)"""
    r = _by_frame(recs[seq])[49]
    target = {bc.REVISIT: (10, 11), bc.SHORT: (20, 21)}[seq]
    assert len(r["ids"]) == 4 and any(int(i) in target for i in r["ids"])
    assert any(0 <= int(i) < 48 for i in r["ids"])
    # one keyframe earlier (max_id = -2) and one later (max_id = 0) only the newest entry is eligible
    assert all(int(i) == 47 for i in _by_frame(recs[seq])[48]["ids"])
    if seq == bc.REVISIT:
        r50 = _by_frame(recs[seq])[50]
        assert len(r50["ids"]) >= 1 and all(int(i) == 49 for i in r50["ids"])


def test_empty_and_stopped_keyframes(recs):
    voc = bc.vocabulary()
    o = bow_util.OracleVoc(voc)
    d = bc.stopped_descriptors()
    w, wt = o.transform(d)
    assert len(d) >= 8 and (wt == 0.0).all() and len(o.bow(d)[0]) == 0
    assert len(o.bow(np.zeros((0, 4), np.uint64))[0]) == 0
    o.close()
    stream = bc.streams()[bc.TIES]
    assert len(stream[bc.EMPTY_STEP][1]) == 0 and stream[bc.EMPTY_STEP][0] == 1 and stream[bc.STOPPED_STEP][0] == 1
    for t in (bc.EMPTY_STEP, bc.STOPPED_STEP):
        r = recs[bc.TIES][t]
        assert len(r["ids"]) == 0 and r["loop"] == -1
    # and neither is ever returned by a later query: an entry without words shares none
    assert not any(int(i) in (bc.EMPTY_STEP, bc.STOPPED_STEP) for r in recs[bc.TIES] if r is not None for i in r["ids"])


def test_eligible_entry_count_passes_a_wavefront(recs):
    """eligible entries of frame f > 50: the f - 50 below the cut-off and the newest one: 63, 64, 65 at frames 112, 113, 114"""
    f = _by_frame(recs[bc.REVISIT])
    for frame, eligible in ((112, 63), (113, 64), (114, 65)):
        assert frame in f and f[frame]["mode"] == 1 and (frame - 50) + 1 == eligible
    assert max(f) < bc.MAX_KEYFRAMES
    # with all results asked for, such a query touches more entries than four
    o = bow_util.OracleVoc(bc.vocabulary())
    for t, (mode, d) in enumerate(bc.streams()[bc.REVISIT]):
        if t == 114:
            ids, _ = o.query(d, 0, t - 50)
            assert len(ids) > 4 and ids.max() == 113
        o.add(d)
    o.close()
