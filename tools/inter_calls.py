"""H.264 inter residual launches (`encode_inter_mb`, and `encode_inter_chroma` right after it) of a
rocprofv3 kernel trace (rocpd SQLite .db) classed by the coding step they belong to, using launch
order as tools/intra_calls.py does: the kernels between one `encode_inter_mb` launch and the
previous one are a step's, and a step with `b_direct_mv` codes B pictures, any other P pictures.

usage: python tools/inter_calls.py <run_results.db> [batches]
       batches: bench steps in the trace, warmup included (default 4), for the per-batch columns
"""
import sqlite3
import statistics
import sys

KERNELS = ("encode_inter_mb", "encode_inter_chroma")


def main():
    c = sqlite3.connect(sys.argv[1])
    batches = int(sys.argv[2]) if len(sys.argv) > 2 else 4
    rows = list(c.execute("select name, start, end from kernels order by start"))
    calls = {k: {"P": [], "B": []} for k in KERNELS}
    seen_b, kind = False, "P"
    for name, st, en in rows:
        k = next((k for k in KERNELS if k in name), None)
        if k is None:
            seen_b = seen_b or "b_direct_mv" in name
            continue
        if k == "encode_inter_mb":  # the chroma launch that follows belongs to the same step
            kind, seen_b = ("B" if seen_b else "P"), False
        calls[k][kind].append((en - st) / 1e3)
    print("| kernel | class | calls per batch | median us | mean us | min | max | ms per batch |")
    print("|---|---|---|---|---|---|---|---|")
    total = 0.0
    for k in KERNELS:
        for cls in ("P", "B"):
            us = calls[k][cls]
            if not us:
                continue
            total += sum(us)
            print(f"| {k} | {cls} | {len(us) / batches:.1f} | {statistics.median(us):.1f} | {statistics.mean(us):.1f} | "
                  f"{min(us):.1f} | {max(us):.1f} | {sum(us) / batches / 1e3:.2f} |")
    print(f"all: {total / batches / 1e3:.2f} ms per batch")


if __name__ == "__main__":
    main()
