#!/usr/bin/env python3
"""Generate tests/golden/pvq_corpus.npz from the REAL reference (oracle/_ref): every run of the
directed PVQ corpus (tests/_pvq_corpus.py; the runs and their order: tests/_pvq_corpus_oracle.py)
through the reference's pvq_theta.  Per run the fixture keeps the recorded results only - the
return value, itheta, max_theta, k and the CRC-32s of `out` and `y` - plus the number of runs and a
digest of the generated inputs, so that a drifted generator fails loudly.  Dev-container only;
deterministic, byte for byte (fixed archive timestamps)."""
import io
import os
import sys
import zipfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
from _libs import GOLDEN, ref  # noqa: E402
import _pvq_corpus_oracle as R  # noqa: E402


def main():
    r = ref()
    assert r is not None, "build oracle/_ref first: make -C oracle ref"
    rows = [R.record(R.theta(r.ref_pvq_theta, x0, r0, n, q0, beta, kf, pli, qm, qmi, trace=False))
            for (_, kf, pli, n, _, x0, r0, q0, beta, qm, qmi) in R.runs()]
    cols = list(zip(*rows))
    d = {"count": np.array(len(rows), "<i4"), "inputs_digest": np.array(R.inputs_digest(), "<u4")}
    for f, col in zip(R.FIELDS, cols):
        d[f] = np.array(col, "<u4" if f.startswith("crc") else "<i4")
    path = os.path.join(GOLDEN, "pvq_corpus.npz")
    with zipfile.ZipFile(path, "w", zipfile.ZIP_DEFLATED, compresslevel=9) as z:
        for name in sorted(d):
            buf = io.BytesIO()
            np.lib.format.write_array(buf, d[name], allow_pickle=False)
            info = zipfile.ZipInfo(name + ".npy", date_time=(1980, 1, 1, 0, 0, 0))
            info.compress_type = zipfile.ZIP_DEFLATED
            info.external_attr = 0o644 << 16
            z.writestr(info, buf.getvalue(), compresslevel=9)
    print("%d runs, inputs digest %08x, %d bytes" % (len(rows), int(d["inputs_digest"]), os.path.getsize(path)))


if __name__ == "__main__":
    main()
