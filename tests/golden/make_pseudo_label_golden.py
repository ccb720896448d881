"""Writes tests/golden/pseudo_label.npz: the REFERENCE's LabelFormatter (utils/label_formatter.py,
imported unchanged; needs the reference sources and scipy) run over pseudo_label_cases.py:
`step` on CPU tensors, `compute`, then `gen_pseudo` scan by scan (not its process pool).
Recorded per case: pseudo_boxes and the array written for every scan.  The generator asserts
that of the boxes past the thresholds the reference keeps at least a quarter and drops at least
a quarter, so neither side of the vote is trivial."""
import os
import sys
import tempfile

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

import pseudo_label_cases as PC  # noqa: E402
from ref_loader import load_reference  # noqa: E402


def main():
    load_reference()
    from utils.label_formatter import LabelFormatter
    out = {}
    for name, cs in PC.CASES.items():
        scans, steps = PC.make(name)
        names = [PC.scan_name(i) for i in range(len(scans))]
        with tempfile.TemporaryDirectory() as tmp:
            lab, dst = os.path.join(tmp, "lseg"), os.path.join(tmp, "out")
            os.makedirs(lab)
            os.makedirs(dst)
            for n, raw in zip(names, scans):
                np.save(os.path.join(lab, n + ".npy"), raw)
            lf = LabelFormatter("", dst, lab, names)
            for outputs, scan_idx in steps:
                lf.step({k: torch.from_numpy(v) for k, v in outputs.items()},
                        {"scan_idx": torch.from_numpy(scan_idx)})
            lf.compute(0, cs["th_s"], cs["th_o"])
            kept = sum(lf.gen_pseudo(i) for i in range(len(names)))
            out[f"{name}/pseudo_boxes"] = lf.pseudo_boxes
            for i, n in enumerate(names):
                out[f"{name}/bbox/{i}"] = np.load(os.path.join(dst, n + "_bbox.npy"))
        cand, past = sum(s[1].size * PC.Q for s in steps), lf.pseudo_boxes.shape[0]
        print(f"{name}: {cand} candidates -> {past} past the thresholds -> {kept} kept, "
              f"{past - kept} dropped; empty files {[i for i in range(len(names)) if not out[f'{name}/bbox/{i}'].shape[0]]}")
        assert 4 * kept >= past and 4 * (past - kept) >= past and past > 0, name
    path = os.path.join(HERE, "pseudo_label.npz")
    np.savez_compressed(path, **out)
    print("wrote", path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
