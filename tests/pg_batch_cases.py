"""Descriptor streams for the batched loop detection (csrc/pg_batch.hip): S = 4 sequences stepped together, each built to reach branches of
PoseGraph::detectLoop and of the database query.  test_pg_batch_cases_cpu.py shows with the oracle alone that every stream reaches what it is
named for; test_gpu_pg_batch.py runs them through one BatchDatabase.  No GPU here, fixed seeds, built from bow_util.place_descriptors / view_of.

A stream is a list of steps; a step is (mode, descriptors): mode 0 = no keyframe for this sequence in this step, 1 = detectLoop (query, then
add), 2 = addKeyFrameIntoVoc (add only).  frame_index of a sequence = the number of keyframes it has added so far."""
import functools

import numpy as np

import bow_util

S = 4
STEPS = 116            # sequence 0 runs all of them (its query reaches 65 eligible entries at frame 114); the others stop near 70
MAX_KEYFRAMES, MAX_KEYPOINTS = 128, 256
REVISIT, SHORT, SPARSE, TIES = 0, 1, 2, 3
EMPTY_STEP, STOPPED_STEP = 10, 11          # in TIES: a keyframe without descriptors, one whose descriptors all fall on stopped words


@functools.lru_cache(maxsize=None)
def vocabulary():
    return bow_util.make_vocabulary(10, 4, 33)


@functools.lru_cache(maxsize=None)
def _places(seq):
    voc = vocabulary()
    return [bow_util.place_descriptors(voc, 1000 * (seq + 1) + p, 150) for p in range(40)]


def _view(seq, place, t):
    return bow_util.view_of(_places(seq)[place], 7000 * (seq + 1) + t, noise_bits=8, extra=40)


@functools.lru_cache(maxsize=None)
def stopped_descriptors():
    """leaf descriptors of stopped words (weight 0) that the tree walk takes back to a stopped word (checked with bow_util.reference_walk)"""
    voc = vocabulary()
    out = []
    for node in voc["word_node"][voc["weight"][voc["word_node"] - 1] == 0.0]:
        d = voc["desc"][node - 1]
        if bow_util.reference_walk(voc, d)[1] == 0.0:
            out.append(d)
        if len(out) == 24:
            break
    assert len(out) >= 8
    return np.ascontiguousarray(np.array(out, np.uint64).reshape(-1, 4))


def _none():
    return np.zeros((0, 4), np.uint64)


@functools.lru_cache(maxsize=None)
def streams():
    """[S] lists of STEPS (mode, descriptors uint64[n][4])"""
    out = [[] for _ in range(S)]
    # REVISIT: two views per place for 52 keyframes, then views of the places of keyframes 0, 1, 2, ... again: by then those keyframes are
    # below the query's cut-off frame_index - 50, so both of a place's views are eligible and the gates open.  Keyframe 49 (cut-off -1:
    # everything eligible) looks at place 5, the place of keyframes 10 and 11.
    for t in range(STEPS):
        place = 5 if t == 49 else (t // 2 if t < 52 else ((t - 52) // 2) % 26)
        out[REVISIT].append((1, _view(REVISIT, place, t)))
    # SHORT: 50 keyframes (frame indices 0 .. 49), new places throughout except keyframe 49, which returns to the place of keyframes 20, 21
    for t in range(STEPS):
        if t < 50:
            out[SHORT].append((1, _view(SHORT, 10 if t == 49 else t // 2, t)))
        else:
            out[SHORT].append((0, _none()))
    # SPARSE: no keyframe on every fourth step, add-only on every fifth, until step 96: the frame index lags the step count.  From keyframe
    # 52 on it revisits like REVISIT.
    k = 0
    for t in range(STEPS):
        if t % 4 == 3 or t >= 96:
            out[SPARSE].append((0, _none()))
            continue
        place = k // 2 if k < 52 else ((k - 52) // 2) % 26
        out[SPARSE].append((2 if t % 5 == 0 else 1, _view(SPARSE, place, t)))
        k += 1
    # TIES: keyframes 0 and 1 are the same view (bit for bit), an empty keyframe, a keyframe on stopped words only, new places up to
    # keyframe 50, keyframe 51 and the later ones views of place 0 again: keyframe 52's query sees keyframes 0 and 1 with equal scores and
    # keyframe 51 as the newest (three results); keyframe 51's sees keyframe 0 and the newest (two), keyframe 50's only the newest (one)
    twin = _view(TIES, 0, 0)
    for t in range(STEPS):
        if t >= 70:
            out[TIES].append((0, _none()))
        elif t in (0, 1):
            out[TIES].append((1, twin))
        elif t == EMPTY_STEP:
            out[TIES].append((1, _none()))
        elif t == STOPPED_STEP:
            out[TIES].append((1, stopped_descriptors()))
        elif t >= 49:
            out[TIES].append((1, _view(TIES, 0, t)))
        else:
            out[TIES].append((1, _view(TIES, 1 + t // 2, t)))
    for seq in out:
        assert len(seq) == STEPS and all(len(d) <= MAX_KEYPOINTS for _, d in seq)
    return out


def replay_oracle(stream, voc=None):
    """one sequence's stream through its own bow_util.OracleVoc: per step None (mode 0) or dict(frame, mode, ids, scores, loop); for mode 2
    ids / scores are empty and loop is -1"""
    o = bow_util.OracleVoc(voc if voc is not None else vocabulary())
    rec, frame = [], 0
    for mode, d in stream:
        if mode == 0:
            rec.append(None)
            continue
        if mode == 1:
            ids, sc = o.query(d, 4, frame - 50)
            loop = o.detect_loop(d, frame)
        else:
            ids, sc, loop = np.zeros(0, np.int32), np.zeros(0), -1
            assert o.add(d) == frame
        rec.append(dict(frame=frame, mode=mode, ids=ids.copy(), scores=sc.copy(), loop=int(loop)))
        frame += 1
    o.close()
    return rec
