"""Class the motion-search dispatches of a rocprofv3 kernel trace (rocpd SQLite .db) of bench.py
as profiles/me_gated_span.md does: ungated list-0[0] searches of P pictures (`me_p16x16<R, 1>`),
gated searches of B pictures (the `me_p16x16<R, 8>` calls after a `b_direct_mv` and before the
picture's `encode_inter_mb`) and gated searches of farther list-0 pictures (every other gated call).

usage: python tools/me_calls.py <run_results.db> STEPS
"""
import re
import sqlite3
import statistics
import sys


def main():
    path, steps = sys.argv[1], int(sys.argv[2])
    c = sqlite3.connect(path)
    rows = list(c.execute("select name, start, end from kernels order by start"))
    cls = {"P list-0[0], no gate": [], "B, gated": [], "farther list-0, gated": [], "me_ref_select": []}
    after_b = False
    for name, st, en in rows:
        if "b_direct_mv" in name:
            after_b = True
        elif "encode_inter_mb" in name:
            after_b = False
        elif "me_ref_select" in name:
            cls["me_ref_select"].append((en - st) / 1e3)
        else:
            m = re.search(r"me_p16x16<\d+, (\d+)>", name)
            if m:
                key = "P list-0[0], no gate" if m.group(1) == "1" else ("B, gated" if after_b else "farther list-0, gated")
                cls[key].append((en - st) / 1e3)
    t0, t1 = rows[0][1], max(r[2] for r in rows)
    print(f"{len(rows)} dispatches over {(t1 - t0) / 1e6:.1f} ms, {steps} steps")
    print("| class | calls per step | mean us | min | median | max | ms per step |")
    print("|---|---|---|---|---|---|---|")
    for k, v in cls.items():
        if v:
            print(f"| {k} | {len(v) / steps:.1f} | {statistics.mean(v):.1f} | {min(v):.1f} | {statistics.median(v):.1f} | "
                  f"{max(v):.1f} | {sum(v) / steps / 1e3:.1f} |")


if __name__ == "__main__":
    main()
