"""GPU Grep map throughput: the warm match pipeline (candidates → selection →
span aggregate → pack, native/kernels/grep.hip) on a seeded ASCII corpus held
in HBM, against text.count_words (the WordCount tokenizer pipeline) on the
same buffer.  Both stream the text once.  Prints one JSON line (GB/s)."""
import argparse
import json
import os
import random
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from hbmr.ops import grep, text  # noqa: E402

PATTERNS = [r"w[1-4]", r"[a-z]+@[a-z]+", r"(foo|foobar)\w*"]


def corpus(mb, seed=7):
    """Lines of 4–16 words over a small vocabulary; one 1 MiB block repeated
    with a per-block salt word so the buffer is not periodic."""
    rnd = random.Random(seed)
    vocab = [f"w{i}" for i in range(2000)] + ["foo", "foobar", "foobarbaz", "the", "of", "and",
                                              "user@example", "a@b", "xyzzy", "lorem", "ipsum"]
    lines, size = [], 0
    while size < 1 << 20:
        ln = " ".join(rnd.choice(vocab) for _ in range(rnd.randint(4, 16))) + "\n"
        lines.append(ln)
        size += len(ln)
    block = "".join(lines).encode()
    return b"".join(b"salt%d " % i + block for i in range(mb))


def timed(fn, reps):
    fn()
    torch.cuda.synchronize()
    best = float("inf")
    for _ in range(reps):
        t = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        best = min(best, time.perf_counter() - t)
    return best


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--mb", type=int, default=256)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--out", default=None, help="also write the JSON line to this file")
    a = ap.parse_args()
    data = corpus(a.mb)
    buf = torch.frombuffer(bytearray(data), dtype=torch.uint8).cuda()
    n = buf.numel()
    res = {"benchmark": "GPU Grep warm map pipeline vs WordCount tokenizer pipeline (1 MI355X)",
           "input_mb": round(n / 2**20, 1), "reps": a.reps, "patterns": {}}
    s = timed(lambda: text.count_words(buf), a.reps)
    res["count_words_ms"] = round(s * 1e3, 2)
    res["count_words_gb_per_s"] = round(n / s / 1e9, 2)
    check = data[:1 << 20]
    check = check[:check.rfind(b"\n") + 1]
    for pat in PATTERNS:
        prog = grep.compile_pattern(pat)
        if prog is None:
            raise SystemExit(f"{pat}: {grep.why_ineligible(pat)}")
        s = timed(lambda: grep.count_matches(buf, prog), a.reps)
        c = timed(lambda: grep.candidates(buf, prog), a.reps)
        blob, counts, _ = grep.count_matches(buf, prog)
        cb, cc, _ = grep.count_matches(buf[:len(check)], prog)
        wb, wc = grep.count_matches_cpu(check, pat)
        ok = dict(text.parse_table(bytes(cb.cpu().numpy()), cc.cpu())) == \
            dict(text.parse_table(bytes(wb.numpy()), wc))
        res["patterns"][pat] = {
            "dfa_states": prog.nstates, "byte_classes": prog.nclasses,
            "matches": int(counts.sum()), "distinct": int(counts.numel()),
            "pipeline_ms": round(s * 1e3, 2), "gb_per_s": round(n / s / 1e9, 2),
            "candidates_only_ms": round(c * 1e3, 2),
            "fraction_of_count_words_rate": round(res["count_words_ms"] / (s * 1e3), 3),
            "first_mib_matches_re": ok}
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
