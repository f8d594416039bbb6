"""H.264 deblocking launches of a rocprofv3 kernel trace (rocpd SQLite .db) classed by the coding
step they belong to, using launch order as tools/intra_calls.py does: the kernels since the
previous `deblock_wavefront` are a step's, and a step with `b_direct_mv` codes B pictures, one with
`p_mv_refine` / `p_part8x8` / `me_ref_select` / `encode_inter_mb` P pictures, one with neither an
I picture.  `deblock_bs` (the pre-pass) is listed on its own.

usage: python tools/deblock_calls.py <run_results.db>
"""
import sqlite3
import statistics
import sys

MARKS = ("b_direct_mv", "p_mv_refine", "p_part8x8", "me_ref_select", "encode_inter_mb")


def main():
    c = sqlite3.connect(sys.argv[1])
    rows = list(c.execute("select name, start, end from kernels order by start"))
    calls, seen = [], set()
    for name, st, en in rows:
        if "deblock_wavefront" in name:
            b, p = "b_direct_mv" in seen, bool(seen & set(MARKS[1:]))
            calls.append(("P+B" if b and p else "B" if b else "P" if p else "I", (en - st) / 1e3))
            seen = set()
        elif "deblock_bs" in name:
            calls.append(("deblock_bs", (en - st) / 1e3))
        else:
            seen.update(k for k in MARKS if k in name)
    n_i = max(1, sum(1 for k, _ in calls if k == "I"))
    print(f"{sum(1 for k, _ in calls if k != 'deblock_bs')} deblock_wavefront launches in {n_i} batches")
    print("| class | calls per batch | mean us | min | median | max | ms per batch |")
    print("|---|---|---|---|---|---|---|")
    for k in ("I", "P", "B", "P+B", "deblock_bs"):
        us = [u for kk, u in calls if kk == k]
        if us:
            print(f"| {k} | {len(us) / n_i:.1f} | {statistics.mean(us):.1f} | {min(us):.1f} | {statistics.median(us):.1f} | "
                  f"{max(us):.1f} | {sum(us) / n_i / 1e3:.2f} |")


if __name__ == "__main__":
    main()
