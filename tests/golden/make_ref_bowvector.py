"""tests/golden/ref_bowvector.npz: what the reference's own DBoW2::BowVector (oracle/ref_bowvector.cpp over the reference's BowVector.cpp,
built into oracle/_ref by `make -C oracle ref` where the reference tree is present) makes of the (word, weight) sequences of
tests/test_oracle_bow_cpu.py::test_bow_vector_against_the_reference_class_itself, per weighting w and view s: the input sequence
(w<w>_s<s>_word, _weight) and the class's normalised vector (_id, _value).    python tests/golden/make_ref_bowvector.py"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import bow_util  # noqa: E402
from test_oracle_bow_cpu import _ref_bowvector  # noqa: E402

R = _ref_bowvector()
assert R is not None, "oracle/_ref/libdbow_bowvector_ref.so is not built (make -C oracle ref needs the reference tree)"
out = {}
for weighting in range(4):
    voc, views = bow_util.ref_bowvector_inputs(weighting)
    o = bow_util.OracleVoc(voc)
    for seed, feats in enumerate(views):
        w, wt = o.transform(feats)
        w32 = np.ascontiguousarray(w, np.int32)
        ids, val = np.zeros(len(w), np.int32), np.zeros(len(w))
        m = R.oref_bow_vector(len(w), w32.ctypes.data, wt.ctypes.data, weighting, len(w), ids.ctypes.data, val.ctypes.data)
        key = "w%d_s%d_" % (weighting, seed)
        out.update({key + "word": w32, key + "weight": wt, key + "id": ids[:m], key + "value": val[:m]})
    o.close()
np.savez_compressed(os.path.join(HERE, "ref_bowvector.npz"), **out)
