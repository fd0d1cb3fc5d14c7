"""The unmodified reference's results on the cases of a tools/ref_diff_*.py run.  Recorded once where the reference is on the box
(`--record`: the tool's child process runs it and the results go to tests/golden/refdiff_<tool>_<cases>_<seed>_part<k>.npz), read back from
that fixture everywhere else -- the CPU suite needs no copy of the reference.  A fixture holds a digest of the cases it was recorded
on: cases generated differently are refused, never compared against another run's answers."""
import hashlib
import os
import pickle
import subprocess
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")


def parse_argv(default_cases):
    """[cases [seed]] [--record] -> (cases, seed, record)."""
    pos = [a for a in sys.argv[1:] if a != "--record"]
    return (int(pos[0]) if pos else default_cases), (int(pos[1]) if len(pos) > 1 else 0), "--record" in sys.argv


def _feed(h, v):
    if isinstance(v, dict):
        for k in sorted(v):
            h.update(repr(k).encode())
            _feed(h, v[k])
    elif isinstance(v, (list, tuple)):
        h.update(b"[%d" % len(v))
        for x in v:
            _feed(h, x)
    elif isinstance(v, np.ndarray):
        h.update(("%s%s" % (v.dtype.str, v.shape)).encode())
        h.update(np.ascontiguousarray(v).tobytes())
    else:
        h.update(repr(v).encode())


def digest(cases):
    h = hashlib.sha256()
    _feed(h, cases)
    return h.hexdigest()


PART_BYTES = 600 << 10          # (random float64 does not compress: a record is split into files well below the 1 MiB limit)


def save(prefix, results, dg):
    """results -> prefix_part0.npz, prefix_part1.npz, ...: cases in order, each part up to PART_BYTES of arrays."""
    parts, z, size = [], None, 0
    for i, r in enumerate(results):
        if z is None or size > PART_BYTES:
            z, size = {"digest": np.array(dg), "count": np.array(len(results))}, 0
            parts.append(z)
        for k, v in r.items():
            a = np.array("") if v is None else np.asarray(v)
            z["%d/%s" % (i, k)] = a
            size += a.nbytes
            if v is None:
                z["%d/%s/none" % (i, k)] = np.array(True)
    for j, z in enumerate(parts):
        np.savez_compressed("%s_part%d.npz" % (prefix, j), **z)


def load(prefix):
    out, dg, j = None, None, 0
    while os.path.exists("%s_part%d.npz" % (prefix, j)):
        with np.load("%s_part%d.npz" % (prefix, j), allow_pickle=False) as z:
            if out is None:
                out, dg = [dict() for _ in range(int(z["count"]))], str(z["digest"])
            assert str(z["digest"]) == dg
            for key in z.files:
                parts = key.split("/")
                if len(parts) != 2:
                    continue
                a = z[key]
                out[int(parts[0])][parts[1]] = None if ("%s/none" % key) in z.files else (a.item() if a.ndim == 0 else a)
        j += 1
    return out, dg


def reference_results(tool, child, cases, n_cases, seed, record):
    """The reference's results on `cases` (one dict per case), or None when there is neither a fixture nor a reference."""
    fixture = os.path.join(GOLDEN, "refdiff_%s_%d_%d" % (tool, n_cases, seed))
    dg = digest(cases)
    if not record and os.path.exists(fixture + "_part0.npz"):
        res, got = load(fixture)
        if got != dg or len(res) != len(cases):
            sys.exit("%s_part*.npz were recorded on other cases than these: record it again (--record, with the reference on the box)" % fixture)
        return res
    ref = os.environ.get("MPC_REFERENCE_DIR", "")
    if not (ref and os.path.isdir(os.path.join(ref, "mpc"))):
        return None
    tmp = tempfile.mkdtemp()
    pickle.dump(cases, open(os.path.join(tmp, "cases.pkl"), "wb"))
    env = dict(os.environ)
    env.pop("PYTHONPATH", None)
    subprocess.check_call([sys.executable, os.path.join(ROOT, "tools", child), os.path.join(tmp, "cases.pkl"), os.path.join(tmp, "ref.pkl")],
                          env=env, cwd=tmp)
    res = pickle.load(open(os.path.join(tmp, "ref.pkl"), "rb"))
    if record:
        save(fixture, res, dg)
        print("recorded %s" % fixture)
    return res
