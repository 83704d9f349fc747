"""Golden vectors for the WER counts (tests/test_decode.py), from the REFERENCE's own
metrics.py: wer_single and wer_list (metrics.py:2754-2907).

Runs ONLY where the reference checkout is importable (SCATTEN_REFERENCE, default
/root/reference).  metrics.py imports `portalocker` at module level (metrics.py:33) for its
sacreBLEU download code, which is never called here; the import is satisfied by an EMPTY
module object registered under that name before `import metrics`.  Every function called below
is the reference's own code, unchanged.

Token ids are mapped to the strings "w<id>" joined by blanks, as the reference scores strings.
Writes `wer_cases.npz` — data only: the padded token rows, their lengths, the reference's
(num_del, num_ins, num_sub, num_ref) per pair, and the wer_list rates over all pairs and over
three subsets that exercise its replacement of zero totals by 1.

Usage:  PYTHONDONTWRITEBYTECODE=1 python tests/golden/gen_golden_wer.py
"""
import os
import sys
import types

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
REF = os.environ.get("SCATTEN_REFERENCE", "/root/reference")

sys.path.insert(0, REF)
sys.modules.setdefault("portalocker", types.ModuleType("portalocker"))  # metrics.py:33, unused here
import metrics as ref_metrics  # noqa: E402

RATES = ("wer", "del_rate", "ins_rate", "sub_rate")
# subsets for wer_list: (name, indices into the cases; None = all)
SUBSETS = (("all", None), ("identical_only", "identical"), ("empty_ref_only", "empty_ref"), ("first_six", 6))


def cases():
    rng = np.random.default_rng(42)
    c = []  # (tag, ref ids, hyp ids)
    c.append(("empty_hyp", [5, 6, 7], []))
    c.append(("empty_ref", [], [3, 4]))
    c.append(("both_empty", [], []))
    c.append(("identical", [1, 2, 3, 4, 5], [1, 2, 3, 4, 5]))
    c.append(("pure_ins", [1, 2, 3], [1, 9, 2, 8, 3, 7]))
    c.append(("pure_del", [1, 2, 3, 4, 5, 6], [2, 4, 6]))
    c.append(("pure_sub", [1, 2, 3, 4], [5, 6, 7, 8]))
    # substitution (4) against deletion + insertion (6), and a cell where they tie in count
    c.append(("sub_vs_del_ins", [1, 2, 3], [1, 4, 3]))
    c.append(("tie_shift", [1, 2, 3, 4], [2, 3, 4, 5]))
    c.append(("tie_swap", [1, 2], [2, 1]))
    c.append(("repeat_tokens", [1, 1, 2, 2, 1], [1, 2, 2, 1, 1]))
    c.append(("len1_same", [7], [7]))
    c.append(("len1_diff", [7], [8]))
    c.append(("len1_vs_many", [7], [1, 2, 7, 3]))
    for k in range(4):
        r = rng.integers(1, 9, 30).tolist()
        h = [t for t in r if rng.random() > 0.2]
        h = [int(rng.integers(1, 9)) if rng.random() < 0.2 else t for t in h]
        for _ in range(int(rng.integers(0, 5))):
            h.insert(int(rng.integers(0, len(h) + 1)), int(rng.integers(1, 9)))
        c.append((f"len30_{k}", r, h[:30]))
    for k in range(3):  # 42 + 42: 3 (R + H) = 252, the reference's uint8 matrix cannot wrap
        r = rng.integers(1, 6 + 20 * k, 42).tolist()
        h = rng.integers(1, 6 + 20 * k, 42).tolist()
        c.append((f"len42_{k}", r, h))
    r = rng.integers(1, 50, 42).tolist()
    c.append(("len42_rotated", r, r[5:] + r[:5]))
    return c


def to_str(ids):
    return " ".join(f"w{int(i)}" for i in ids)


def main():
    cs = cases()
    N = len(cs)
    Rmax = max(len(r) for _, r, _ in cs)
    Hmax = max(len(h) for _, _, h in cs)
    ref = np.zeros((N, Rmax), np.int32)
    hyp = np.zeros((N, Hmax), np.int32)
    ref_len = np.zeros(N, np.int32)
    hyp_len = np.zeros(N, np.int32)
    counts = np.zeros((N, 4), np.int32)
    for n, (_, r, h) in enumerate(cs):
        assert 3 * (len(r) + len(h)) <= 255
        ref[n, :len(r)], hyp[n, :len(h)], ref_len[n], hyp_len[n] = r, h, len(r), len(h)
        res = ref_metrics.wer_single(r=to_str(r), h=to_str(h))
        counts[n] = [res["num_del"], res["num_ins"], res["num_sub"], res["num_ref"]]
        assert res["num_err"] == res["num_del"] + res["num_ins"] + res["num_sub"]
    tags = [t for t, _, _ in cs]
    out = {"ref": ref, "ref_len": ref_len, "hyp": hyp, "hyp_len": hyp_len, "counts": counts,
           "tags": np.array(tags)}
    for name, pick in SUBSETS:
        idx = (list(range(N)) if pick is None else list(range(pick)) if isinstance(pick, int)
               else [tags.index(pick)])
        res = ref_metrics.wer_list(references=[to_str(cs[i][1]) for i in idx],
                                   hypotheses=[to_str(cs[i][2]) for i in idx])
        out[f"subset_{name}_idx"] = np.array(idx, np.int64)
        out[f"subset_{name}_rates"] = np.array([res[k] for k in RATES], np.float64)
    np.savez_compressed(os.path.join(HERE, "wer_cases.npz"), **out)
    print(N, "cases", ref.shape, hyp.shape)


if __name__ == "__main__":
    main()
