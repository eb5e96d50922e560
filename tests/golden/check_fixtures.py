"""Do the committed generators still produce the committed fixtures?  Runs every tests/golden/gen_*_fixtures.py as a child process
writing to a temporary directory (ref_harness.OUT_ENV), then compares each file with the committed one byte for byte; a committed
.npz that no generator produced, or a produced one that is not committed, is a mismatch too.

usage: python tests/golden/check_fixtures.py
exit status: 0 all agree; 1 a generator failed or a file differs (each named, with its first differing array); 3 (NO_REFERENCE) the
reference checkout (ref_harness.REF) is absent, so nothing could be generated."""
import glob
import os
import subprocess
import sys
import tempfile

import numpy as np

import ref_harness as rh

NO_REFERENCE = 3


def first_difference(got, want):
    """What differs between two .npz files, by the first array that does."""
    a, b = np.load(got), np.load(want)
    if a.files != b.files:
        return f"arrays {[k for k in a.files if k not in b.files]} added, {[k for k in b.files if k not in a.files]} missing, or reordered"
    for k in a.files:
        x, y = a[k], b[k]
        if x.shape != y.shape or x.dtype != y.dtype:
            return f"{k}: {x.shape} {x.dtype}, committed {y.shape} {y.dtype}"
        if not np.array_equal(x, y, equal_nan=x.dtype.kind == "f"):
            return f"{k} {x.shape} {x.dtype}: {int((x != y).sum())} of {x.size} elements differ"
    return "same arrays, another container (compression or zip metadata)"


def main():
    if not os.path.isdir(rh.REF):
        print(f"no reference checkout at {rh.REF} (LG_REFERENCE): the fixtures cannot be regenerated here")
        return NO_REFERENCE
    bad = []
    with tempfile.TemporaryDirectory() as out:
        env = dict(os.environ, PYTHONDONTWRITEBYTECODE="1", **{rh.OUT_ENV: out})
        scripts = sorted(glob.glob(os.path.join(rh.GOLDEN, "gen_*_fixtures.py")))
        children = [subprocess.Popen([sys.executable, s], env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
                    for s in scripts]
        for s, c in zip(scripts, children):
            log = c.communicate()[0]
            if c.returncode:
                bad.append(f"{os.path.basename(s)}: exit status {c.returncode}\n{log}")
        made = {f for f in os.listdir(out) if f.endswith(".npz")}
        committed = {os.path.basename(f) for f in glob.glob(os.path.join(rh.GOLDEN, "*.npz"))}
        bad += [f"{f}: committed, but no generator produced it" for f in sorted(committed - made)]
        bad += [f"{f}: produced, but not committed" for f in sorted(made - committed)]
        for f in sorted(made & committed):
            got, want = os.path.join(out, f), os.path.join(rh.GOLDEN, f)
            if open(got, "rb").read() != open(want, "rb").read():
                bad.append(f"{f}: {first_difference(got, want)}")
    print("\n".join(bad) if bad else f"{len(made)} fixtures of {len(scripts)} generators: byte-identical to the committed files")
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
