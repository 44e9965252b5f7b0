#!/usr/bin/env python
"""Writes the fixture of tests/test_gpu_snapshot.py::test_layout_matches_the_recorded_table: the snapshot layout table of a two-sequence
handle for each configuration of LAYOUT_CONFIGS, and the SHA-256 of one saved blob per flavour.  Run it with the library of the commit
whose layout is to be pinned; run it twice (two processes) and commit blob hashes only when both runs agree.
    python tools/record_snapshot_layout.py <commit> out.json [--no-blob]"""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import vio_ct  # noqa: E402
import test_gpu_snapshot as T  # noqa: E402


def main():
    commit, out = sys.argv[1], sys.argv[2]
    P = vio_ct.pkg()
    doc = {"header": "written by tools/record_snapshot_layout.py with the library built from commit %s; rows are [name, kind, bytes per "
                     "sequence, offset in the blob's device part or -1] of VioBatch(canonical_config(**key), 2).snapshot_layout()" % commit,
           "abi_version": int(P.lib().vio_abi_version()), "format_version": int(P.SNAPSHOT_FORMAT),
           "layouts": {T._layout_key(kw): T._layout_rows(P, kw) for kw in T.LAYOUT_CONFIGS},
           "blob_sha256": {} if "--no-blob" in sys.argv else {f: T._blob_sha256(P, f) for f in ("default", "dynamic_init")}}
    with open(out, "w") as f:   # one table row per line
        lay = ",\n".join(' "%s": [\n  %s]' % (k, ",\n  ".join(json.dumps(r) for r in rows)) for k, rows in doc["layouts"].items())
        f.write('{"header": %s,\n"abi_version": %d, "format_version": %d,\n"blob_sha256": %s,\n"layouts": {\n%s}}\n'
                % (json.dumps(doc["header"]), doc["abi_version"], doc["format_version"], json.dumps(doc["blob_sha256"]), lay))


if __name__ == "__main__":
    main()
