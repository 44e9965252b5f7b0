"""The generated tracker streams (tests/tracker_cases.py) on the oracle alone: every case REACHES the branch it is named for, read off the
per-frame trace of Tracker::readImage (oracle.h Tracker::Trace), so that the GPU comparison of tests/test_gpu_tracker_edges.py cannot pass
on a stream that never takes the path.  The figure observed on the oracle stands in a comment beside every bound."""
import numpy as np
import pytest

import tracker_cases as TC
import vio_ct


def _traces(P, name):
    c, recs = TC.oracle_run(name, P)
    return c, recs, [r["trace"] for r in recs]


def _cells(tr):
    return [c for t in tr if t is not None for c in t["cells"]]


def _hw(r):
    hw = np.zeros(r + 1, np.int32)
    vio_ct.oracle().ovio_circle_hw(r, hw.ctypes.data)
    return hw


def decisive_pairs(sm, r):
    """setMask's candidates in sorted order (x, y, track_cnt, kept): the pairs (i, j), i < j, where j was dropped and i is the ONLY kept candidate
    whose disk covers j -- the decision about j hangs on the conflict bit (i, j) alone"""
    hw, out = _hw(r), []
    for j in range(len(sm)):
        if sm[j, 3]:
            continue
        cov = [i for i in range(j) if sm[i, 3] and abs(sm[j, 1] - sm[i, 1]) <= r and abs(sm[j, 0] - sm[i, 0]) <= hw[abs(sm[j, 1] - sm[i, 1])]]
        if len(cov) == 1:
            out.append((cov[0], j))
    return out


# ------------------------------------------------------------------------------------------------------------- hooks
@pytest.mark.parametrize("name", TC.NAMES)
def test_track_output_is_the_map_of_the_tracks_and_hooks_are_inert(P, name):
    """Pipeline::track's feature map (once init_pub / init_feature let it through) equals the map rebuilt from the tracker's state; the trace
    agrees with the state; a bare Tracker with the hooks untouched computes the same state as the Pipeline's"""
    c, recs, tr = _traces(P, name)
    bare = vio_ct.OracleTracker(c.cfg) if c.fisheye is None and c.fast_cap == 0 else None
    n_out = 0
    for f, r in enumerate(recs):
        ids, obs = r["track_out"]
        if len(ids):
            n_out += 1
            assert np.array_equal(ids, r["packaged"][0]) and np.array_equal(obs, r["packaged"][1]), (name, f)
        if r["mode"] == TC.SKIP:
            continue
        t = r["trace"]
        assert t["publish"] == (r["mode"] == TC.PUBLISH)
        added = sum(cl["added"] for cl in t["cells"])
        assert len(r["tracks"][0]) == (t["n_mask"] + added if t["publish"] else t["n_culled"]), (name, f)
        assert t["n_lk"] == (len(recs[f - 1]["tracks"][0]) if f else 0)
        assert len(t["setmask"]) == (t["n_ransac"] if t["publish"] else 0) and int(t["setmask"][:, 3].sum()) == t["n_mask"]
        if bare is not None:
            bare.read(c.frames[f], c.stamps[f], np.eye(3), r["mode"] == TC.PUBLISH)
            for a, b in zip(bare.tracks(), r["tracks"]):
                assert np.array_equal(a, b), (name, f)
            assert bare.trace()["cells"] == t["cells"]
    assert n_out >= 1, name


def test_fast_cap_only_acts_when_set_and_exceeded(P):
    c = TC.build("fast_overflow", P)
    off, huge, cap = TC.run_oracle(c, fast_cap=0), TC.run_oracle(c, fast_cap=1 << 20), TC.run_oracle(c, fast_cap=1024)
    for a, b in zip(off, huge):
        for x, y in zip(a["tracks"], b["tracks"]):
            assert np.array_equal(x, y)
    assert off[2]["trace"]["cells"][0]["nf"] > 1024 >= cap[2]["trace"]["cells"][0]["nf"]      # 4751 against 1010
    assert not np.array_equal(off[2]["tracks"][2], cap[2]["tracks"][2])                         # the truncation changes what is kept
    for f in (0, 1):
        assert np.array_equal(off[f]["tracks"][2], cap[f]["tracks"][2])


# ------------------------------------------------------------------------------------------------------------- fe_add: top-k and addPoints
def test_serial_topk_reaches_the_serial_scan_and_saturates(P):
    for name, cells, K, n_after in (("serial_topk", 1, 152, 152), ("serial_topk_2cells", 2, 77, 154), ("serial_topk_amps", 1, 152, 152)):
        c, recs, tr = _traces(P, name)
        assert len(tr[0]["cells"]) == cells
        for cl in tr[0]["cells"]:
            assert cl["nf"] > cl["num_to_add"] > 64 and cl["num_to_add"] == K          # nf 660 (330 per cell of two), K 152 (77)
            assert cl["added"] == K
        assert len(recs[0]["tracks"][0]) == n_after
        assert all(t["n_max_cnt"] <= 0 and not t["cells"] for t in tr[1:])             # -2 (-4): saturated, no detection at all
    assert all(cl["replacements"] == 0 for cl in _traces(P, "serial_topk")[2][0]["cells"])     # every response tied: the scan never replaces
    amps = _traces(P, "serial_topk_amps")[2][0]["cells"][0]
    assert amps["replacements"] >= 100 and amps["tied_min"] >= 1                       # 182 replacements, 1 of them onto a tied minimum behind an equal slot


def test_wave_topk_reaches_the_wavefront_scan_with_ties(P):
    ties = _traces(P, "wave_topk_ties")[2][0]["cells"][0]
    assert ties["nf"] > ties["num_to_add"] == 62 and ties["replacements"] == 0         # nf 660, K 62 <= 64, all equal: nothing beats the minimum
    amps = _traces(P, "wave_topk_amps")[2][0]["cells"][0]
    assert amps["nf"] > amps["num_to_add"] == 62
    assert amps["replacements"] >= 50 and amps["tied_min"] >= 1                        # 69 replacements, 1 onto a tied minimum behind an equal slot
    assert _traces(P, "wave_topk_amps")[2][1]["n_max_cnt"] <= 0


def test_serial_addpoints_reaches_the_one_by_one_walk(P):
    cl = _traces(P, "serial_addpoints")[2][0]["cells"][0]
    assert 64 < cl["nf"] <= cl["num_to_add"] and cl["added"] == cl["nf"]               # nf 108, K 152
    cl = _traces(P, "serial_addpoints_conflicts")[2][0]["cells"][0]
    assert 64 < cl["nf"] <= cl["num_to_add"] and 64 < cl["added"] < cl["nf"]           # nf 144, K 152, 108 added: the walk rejects 36
    cl = _traces(P, "near_cap")[2][3]["cells"][0]
    assert 64 < cl["nf"] <= cl["num_to_add"]                                           # nf 75 with 300 old centres in the mask


def test_near_cap_overflows_the_short_list_of_old_centres(P):
    c, recs, tr = _traces(P, "near_cap")
    hit = [t for t in tr if t["cells"] and t["max_near"] > 192]
    assert len(hit) >= 2 and max(t["max_near"] for t in hit) >= 300                    # 300 centres reach into the cell on frames 1 and 3
    assert any(cl["added"] > 0 for t in hit for cl in t["cells"])                      # and frame 3 still adds 75 points between them


def test_fast_overflow_exceeds_the_candidate_buffer(P):
    c, recs, tr = _traces(P, "fast_overflow")
    over = [f for f, t in enumerate(tr) if any(cl["n_fast"] > 1024 for cl in t["cells"])]
    assert over == [2] and tr[2]["cells"][0]["n_fast"] >= 4000                          # 4843 survivors on the noise frame only
    assert tr[2]["cells"][0]["nf"] > tr[2]["cells"][0]["num_to_add"] > 64              # 1010 of the first 1024 pass the mask, K 134
    assert tr[2]["cells"][0]["added"] > 0


# ------------------------------------------------------------------------------------------------------------- fe_select: setMask
def test_mask_blocks_reaches_every_block_size(P):
    c, recs, tr = _traces(P, "mask_blocks")
    assert [t["n_ransac"] for t in tr] == [0, 1, 63, 64, 65, 128, 129, 216, 216]       # n into setMask, frame by frame
    assert all(t["n_mask"] == t["n_ransac"] for t in tr)                                # isolated blobs: nothing collides here


def test_mask_collisions_straddle_part_word_and_block_boundaries(P):
    for name, tied in (("mask_collide_equal", True), ("mask_collide_mixed", False)):
        c, recs, tr = _traces(P, name)
        part = word = high = block = 0
        for t in tr:
            sm = t["setmask"]
            for i, j in decisive_pairs(sm, c.cfg.min_dist):
                assert (sm[i, 2] == sm[j, 2]) == tied, (name, i, j)        # equal: the pair is ordered by the stable tie rule alone; mixed: old before fresh
                same = i // 64 == j // 64
                part += same and (i % 64) // 16 != (j % 64) // 16
                word += same and i % 64 < 32 <= j % 64
                high += same and i % 64 >= 32            # the conflict bit sits in the HIGH 32-bit word of candidate j's row
                block += not same
        # equal: 120 decisive pairs, 4 across a part, 1 across the word, 1 across a block boundary; mixed: 30 pairs, 18 / 15 / 12
        assert part >= 1 and word >= 1 and high >= 1 and block >= 1, (name, part, word, high, block)
        assert max(len(t["setmask"]) for t in tr) >= 190                    # 300 / 190 candidates: three to five blocks of 64


# ------------------------------------------------------------------------------------------------------------- state machines
def test_ransac_threshold_both_sides(P):
    c, recs, tr = _traces(P, "ransac_7_8")
    assert (tr[1]["n_culled"], tr[1]["ransac_ran"]) == (7, 0) and (tr[2]["n_culled"], tr[2]["ransac_ran"]) == (8, 1)
    assert (tr[3]["n_culled"], tr[3]["ransac_ran"]) == (9, 1)


def test_all_lost_empties_the_tracker_and_ids_continue(P):
    c, recs, tr = _traces(P, "all_lost")
    assert tr[2]["n_lk"] >= 50 and tr[2]["n_culled"] == 0 and tr[2]["n_unstable"] == tr[2]["n_lk"]     # 70 tracks die on the second flat frame
    assert len(recs[2]["tracks"][0]) == 0
    ids, cnt, cur, un, vel = recs[3]["tracks"]
    assert len(ids) == 108 and ids.min() == 108 and np.all(cnt == 1) and not vel.any()                 # ids go on from 108, the map was empty
    assert tr[1]["cells"][0]["textureless"] == 1 and tr[2]["cells"] == [] and tr[3]["cells"][0]["added"] == 108


def test_flat_first_goes_textureless_and_recovers(P):
    c, recs, tr = _traces(P, "flat_first")
    assert [cl["textureless"] for cl in tr[0]["cells"]] == [1, 1, 1, 1] and tr[1]["cells"] == [] and tr[1]["n_max_cnt"] > 0
    assert [cl["cell"] for cl in tr[4]["cells"]] == [0, 1, 2, 3] and all(cl["added"] >= 20 for cl in tr[4]["cells"])   # 35 25 28 20


def test_unstable_points_block_the_new_blobs(P):
    c, recs, tr = _traces(P, "unstable")
    assert tr[2]["n_unstable"] >= 50 and tr[2]["cand_in_unstable"] >= 50                # 52 and 52
    assert len(tr[2]["cells"]) == 1 and tr[2]["cells"][0]["n_fast"] >= 100 and tr[2]["cells"][0]["added"] == 0   # 109 candidates, none added
    assert tr[4]["cells"][0]["added"] == tr[2]["cand_in_unstable"]                      # once the disks are gone the same blobs come in


def test_modes_stream_crowds_through_track_frames(P):
    c, recs, tr = _traces(P, "modes")
    assert c.modes[:6] == [TC.PUBLISH, TC.TRACK, TC.TRACK, TC.PUBLISH, TC.SKIP, TC.PUBLISH]
    assert tr[1]["publish"] == 0 and tr[2]["publish"] == 0 and tr[4] is None
    assert tr[3]["n_lk"] > c.cfg.max_cnt and tr[3]["n_mask"] < tr[3]["n_ransac"] - 30   # 202 tracks into the PUBLISH frame, setMask leaves 137
    assert len(decisive_pairs(tr[3]["setmask"], c.cfg.min_dist)) >= 30                  # 65
    cl = tr[3]["cells"][0]
    assert cl["nf"] > cl["num_to_add"] > 64 and cl["replacements"] >= 10                # nf 108, K 65, 30 replacements
    for a, b in zip(recs[4]["tracks"], recs[3]["tracks"]):
        assert np.array_equal(a, b)                                                     # SKIP leaves the state alone


# ------------------------------------------------------------------------------------------------------------- geometry
def test_exits_touch_the_rounding_limit_of_every_border(P):
    c, recs, tr = _traces(P, "exits")
    h = np.sum([t["border_hits"] for t in tr], 0)
    assert np.all(h[:4] >= 1) and np.count_nonzero(h[4:]) >= 3, h                       # x: 15 2 8 5 at 0, 1, W-2, W-1; y: 1 21 1 0
    assert sum(t["n_lk"] - t["n_culled"] for t in tr) >= 30                             # 49 tracks leave in all
    cells = [cl for t in tr for cl in t["cells"]]
    assert sum(cl["tied_min"] for cl in cells) >= 5 and sum(cl["replacements"] for cl in cells) >= 40   # 11 of 77 replacements onto a tied minimum:
    # the stream that catches a wavefront scan without its `resp == cand_resp` rule


def test_grid_remainder_bands_hold_tracked_points(P):
    c, recs, tr = _traces(P, "grid_remainder")
    assert (c.cfg.width // c.cfg.grid_cols, c.cfg.height // c.cfg.grid_rows) == (63, 47)
    assert max(t["n_col_band"] for t in tr) >= 3 and max(t["n_row_band"] for t in tr) >= 3 and max(t["n_corner_band"] for t in tr) >= 1   # 5, 7, 1
    assert any(t["n_col_band"] and t["cells"] for t in tr)                              # while the grid is counted for a detection


def test_grid_remainder_band_point_decides_the_cells_deficit(P):
    """grids_threshold 1: on frame 4 the ONLY track of cells 3, 12 and 15 sits in the band (col == grid_cols, row == grid_rows or both before the
    decrement).  Counted in its own cell, the cell is full: it is absent from the deficit list although a fresh blob lies in it and the other
    cells detect; the blob comes in on frame 5, when the track has left through the border.  Counted in any other cell, 3 / 12 / 15 would detect
    on frame 4 and take the blob a frame early: a kernel without --col / --row cannot equal the oracle on this stream."""
    c, recs, tr = _traces(P, "grid_remainder_decides")
    assert c.cfg.max_cnt // (c.cfg.grid_rows * c.cfg.grid_cols) == 1
    t = tr[4]
    assert (t["n_mask"], t["n_col_band"], t["n_row_band"], t["n_corner_band"]) == (3, 2, 2, 1)      # every track is a band point
    deficit = {cl["cell"] for cl in t["cells"]}
    assert t["n_max_cnt"] > 0 and deficit == set(range(16)) - {3, 12, 15}, deficit                   # 13 cells detect, the three full ones do not
    assert len(recs[4]["tracks"][0]) == 3 and len(c.frames) == 8
    cur = recs[4]["tracks"][2]
    assert sorted((int(x) // 63, int(y) // 47) for x, y in cur) == [(0, 4), (4, 0), (4, 4)]          # before the decrement: outside the 4 x 4 grid
    late = {cl["cell"]: cl for cl in tr[5]["cells"]}
    assert set(late) >= {3, 12, 15} and all(late[k]["added"] >= 1 for k in (3, 12, 15))               # 2, 2, 1 points added once the tracks have left
    assert tr[5]["n_lk"] == 3 and tr[5]["n_culled"] == 0


@pytest.mark.parametrize("kind", ["wave", "serial", "addpoints"])
def test_fisheye_grey_candidates_on_all_three_values(P, kind):
    c, recs, tr = _traces(P, "fisheye_grey_" + kind)
    t = tr[0]
    assert min(t["cand_fish0"], t["cand_fish_grey"], t["cand_fish255"]) >= 30           # 220 260 180 (36 42 30 on the 20 px lattice)
    cl = t["cells"][0]
    assert t["grey_to_add"] >= 30 and 0 < cl["added"] < min(cl["nf"], cl["num_to_add"])  # 32 / 80 / 42 grey candidates take slots and are refused
    assert cl["nf"] == t["cand_fish_grey"] + t["cand_fish255"]                          # the filter keeps grey, addPoints does not
    assert any(x["n_mask"] < x["n_ransac"] for x in tr[1:])                             # tracks drifting onto grey / black are dropped by setMask
    path = dict(wave=cl["nf"] > cl["num_to_add"] <= 64, serial=cl["nf"] > cl["num_to_add"] > 64, addpoints=64 < cl["nf"] <= cl["num_to_add"])
    assert path[kind]
