"""The tables of oracle/ref_gpu/PINNED.md from a log of tests/test_reference_kernels_gpu.py run with `pytest -s`: every
`PINNED {json}` line is one (case, pair) measurement, printed by the tests before they assert.

    python -m pytest tests/test_reference_kernels_gpu.py -m gpu -s -q > run.log
    python tools/pinned_table.py run.log
"""
import json
import sys

PAIRS = ("R-O", "K-R", "Kculled-R", "Rfma-O")


def fmt(x):
    return "–" if x is None else (f"{x:.1e}" if isinstance(x, float) else str(x))


def main(path):
    cases, knn = {}, []
    with open(path) as f:
        for line in f:
            if "PINNED " not in line:
                continue
            r = json.loads(line[line.index("PINNED ") + 7:])
            if r["pair"] == "knn":
                knn.append(r)
            else:
                cases.setdefault(r["case"], {}).setdefault(r["pair"], {}).update(r)
    for title, backward in (("Forward cases", False), ("Backward cases: the forward of the same frame, and the gradients", True)):
        print(f"\n### {title}\n")
        head = ["case", "pair", "instances", "radii", "tiles_touched", "point_list", "n_contrib", "geometry words", "image mean",
                "image max", "pixels > 1e-5"] + (["worst gradient norm", "worst gradient row"] if backward else [])
        print("| " + " | ".join(head) + " |\n|" + "---|" * len(head))
        for case, pairs in cases.items():
            if case.startswith("bwd/") != backward:
                continue
            for pair in PAIRS:
                r = pairs.get(pair)
                if r is None:
                    continue
                inst = f"{r['R'][0]} / {r['R'][1]}" if r["R"][0] != r["R"][1] else str(r["R"][0])
                row = [case.replace("bwd/", ""), pair, inst] + [fmt(r.get(k)) for k in ("radii", "tiles_touched", "point_list", "n_contrib",
                                                                                   "geom_bits", "img_mean", "img_max", "img_over")]
                if backward:
                    row += [f"{r[k][0]} {fmt(r[k][1])}" if k in r else "–" for k in ("grad_norm", "grad_row")]
                print("| " + " | ".join(row) + " |")
    print("\n### distCUDA2\n\n| cloud | R–O words differing | K–R words differing |\n|---|---|---|")
    for r in knn:
        print(f"| {r['case']} | {r['R_O']} | {r['K_R']} |")


if __name__ == "__main__":
    main(sys.argv[1])
