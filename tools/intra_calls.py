"""H.264 intra launches of a rocprofv3 kernel trace (rocpd SQLite .db) classed by the coding
step they belong to, using launch order: the kernels between one intra launch and the next are
a step's, and a step with `b_direct_mv` codes B pictures, one with `p_mv_refine` / `p_part8x8`
P pictures (both: slots of either kind share the step), one with neither an I picture.  The
`encode_intra_free` and `encode_intra_wavefront` launches of one step are added together.
Calls longer than ten times their class's median are listed with their position (step of the
batch) and what share of them other kernels overlapped.

usage: python tools/intra_calls.py <run_results.db>
"""
import sqlite3
import statistics
import sys

MARKS = ("b_direct_mv", "p_mv_refine", "p_part8x8", "me_ref_select", "encode_inter_mb")


def main():
    c = sqlite3.connect(sys.argv[1])
    rows = list(c.execute("select name, start, end from kernels order by start"))
    steps, seen, cur, first = [], set(), 0.0, None
    for name, st, en in rows:
        if "encode_intra_free" in name or "encode_intra_wavefront" in name:
            cur += (en - st) / 1e3
            first = st if first is None else first
            if "encode_intra_wavefront" in name:
                b, p = "b_direct_mv" in seen, bool(seen & {"p_mv_refine", "p_part8x8", "me_ref_select"})
                kind = "P+B" if b and p else "B" if b else "P" if p or "encode_inter_mb" in seen else "I"
                steps.append((kind, cur, first, en))
                seen, cur, first = set(), 0.0, None
        else:
            seen.update(k for k in MARKS if k in name)
    n_i = max(1, sum(1 for s in steps if s[0] == "I"))
    print(f"{len(steps)} intra launches in {n_i} batches")
    print("| class | calls per batch | mean us | min | median | p90 | max | ms per batch | ms per batch without the long calls |")
    print("|---|---|---|---|---|---|---|---|---|")
    long_calls = []
    for k in ("I", "P", "B", "P+B"):
        us = [s[1] for s in steps if s[0] == k]
        if not us:
            continue
        med = statistics.median(us)
        keep = [u for u in us if u <= 10 * med]
        long_calls += [(i, s) for i, s in enumerate(steps) if s[0] == k and s[1] > 10 * med]
        print(f"| {k} | {len(us) / n_i:.1f} | {statistics.mean(us):.1f} | {min(us):.1f} | {med:.1f} | "
              f"{sorted(us)[int(0.9 * (len(us) - 1))]:.1f} | {max(us):.1f} | {sum(us) / n_i / 1e3:.2f} | "
              f"{statistics.mean(keep) * len(us) / n_i / 1e3:.2f} |")
    i_at = [i for i, s in enumerate(steps) if s[0] == "I"]
    for i, (k, us, st, en) in long_calls:
        cov = sum(max(0, min(en, e) - max(st, s)) for n, s, e in rows if e > st and s < en and "encode_intra" not in n)
        print(f"long {k} call: {us:.0f} us, step {i - max([j for j in i_at if j <= i], default=0)} of its batch, "
              f"other kernels ran during {100 * min(cov, en - st) / max(1, en - st):.0f} % of it")


if __name__ == "__main__":
    main()
