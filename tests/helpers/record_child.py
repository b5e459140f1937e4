"""Child process of tests/test_gpu_batch_record.py::test_two_finishes: USAC_H16_DEFER is read once per
process, so the h16 scorer's own finish (k_h16_finish + the plain argmax) needs a process of its own.

usage: record_child.py IN.npz OUT.npz -- IN holds pts, thr and the sample batches batch0, batch1, ...;
OUT receives per batch counts<i>, sums<i> and the record's fields (hyp<i>, inl<i>, score<i>, model<i>,
valid<i>), floats as int32 bits."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)


def run_batches(usac, pts, thr, batches, first_hyp):
    out = {}
    with usac.Context(usac.ESTIMATOR.Homography, pts) as ctx:
        ctx.set_score_chunks(8)
        for i, smp in enumerate(batches):
            _, _, rec = ctx.hypothesize_score(samples=smp, thr=thr, first_hyp=first_hyp, per_hypothesis=False)
            c, s = ctx.last_counts(len(smp))
            out["counts%d" % i] = c
            out["sums%d" % i] = s.view(np.int32)
            out["hyp%d" % i] = np.uint64(rec["hyp_index"])
            out["inl%d" % i] = np.int32(rec["inliers"])
            out["score%d" % i] = np.array([rec["score"]], np.float32).view(np.int32)
            out["model%d" % i] = rec["model"].view(np.int32)
            out["valid%d" % i] = np.int32(rec["valid"])
    return out


def main():
    import ransac_amd as usac
    z = np.load(sys.argv[1])
    n = sum(1 for k in z.files if k.startswith("batch"))
    pts = [z["pts%d" % i] for i in range(n)]
    out = {}
    for i in range(n):
        r = run_batches(usac, pts[i], float(z["thr"]), [z["batch%d" % i]], int(z["first_hyp"]))
        out.update({k[:-1] + str(i): v for k, v in r.items()})
    np.savez(sys.argv[2], **out)


if __name__ == "__main__":
    main()
