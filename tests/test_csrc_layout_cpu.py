"""How csrc/ is laid out: every header compiles on its own, and a translation unit includes the project's headers at its top only (a header pasted in
further down works by what the unit defined above it, which is how be_kernels.hip once held 9 700 lines together by include order)."""
import glob
import os
import re
import subprocess

CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "vins-rgbd-fast_amd", "csrc")


def test_every_header_stands_alone():
    """csrc/Makefile target `headers`: for each *.h a unit that is that one #include passes hipcc -fsyntax-only (front end only, no code generated)."""
    r = subprocess.run(["make", "-j8", "-C", CSRC, "headers"], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    for h in glob.glob(os.path.join(CSRC, "*.h")):
        assert '#include "%s"' % os.path.basename(h) in r.stdout, "the target did not check " + h


def _code_lines(text):
    """(line number, line) of what is neither blank nor comment"""
    text = re.sub(r"/\*.*?\*/", lambda m: "\n" * m.group(0).count("\n"), text, flags=re.S)
    for n, line in enumerate(text.split("\n"), 1):
        line = line.split("//")[0].strip()
        if line:
            yield n, line


def test_units_include_project_headers_at_the_top_only():
    units = sorted(glob.glob(os.path.join(CSRC, "*.hip")))
    assert units
    late = []
    for u in units:
        below = False
        for n, line in _code_lines(open(u).read()):
            if re.match(r'#\s*include\b', line):
                if below and '"' in line:
                    late.append("%s:%d %s" % (os.path.basename(u), n, line))
            else:
                below = True
    assert not late, late
