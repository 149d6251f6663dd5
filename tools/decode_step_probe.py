"""Graphed decode step of one random-init engine at long context, with and
without a sliding window, and single-shot prefill attention at the same
head geometry. tools/decode_breakdown.py is fixed to llama-3-8b at 8k; this
probe takes the arch, the contexts, the windows and the cache formats.

    decode_step_probe.py [--arch mistral-7b] [--ctx 16384,32000]
                         [--windows 0,4096] [--kv-dtypes bf16,fp8]
                         [--cache 32768] [--prefill-tokens 16384]

Per (cache format, window) one engine is built with the spec keys `kv_dtype`
and `sliding_window`, a cache of `--cache` positions is allocated (its
contents are not prefilled: this times the step, it checks nothing), and for
each context one `decode_step_ws` at that position is captured into a HIP
graph and replayed: 5 warm-up replays, then 100 between two device events,
twice. `--prefill-tokens N` (0 = skip) first times `ops.attn_prefill` on
q [N, hq, hd], k, v [N, kh, hd] per window, 10 calls per figure, twice.
"""
import argparse
import os
import sys

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
import torch  # noqa: E402

from adversarial_spec_amd import ops  # noqa: E402
from adversarial_spec_amd.engine.local import LocalEngine  # noqa: E402
from adversarial_spec_amd.models import get_config  # noqa: E402


def timed(fn, iters, warmup=5):
    """Mean ms per call between two device events."""
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    t0 = torch.cuda.Event(enable_timing=True)
    t1 = torch.cuda.Event(enable_timing=True)
    t0.record()
    for _ in range(iters):
        fn()
    t1.record()
    torch.cuda.synchronize()
    return t0.elapsed_time(t1) / iters


def ints(text):
    return [int(x) for x in text.split(",") if x]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--arch", default="mistral-7b")
    ap.add_argument("--ctx", type=ints, default=[16384, 32000])
    ap.add_argument("--windows", type=ints, default=[0, 4096])
    ap.add_argument("--kv-dtypes", default="bf16,fp8")
    ap.add_argument("--cache", type=int, default=32768)
    ap.add_argument("--prefill-tokens", type=int, default=16384)
    args = ap.parse_args()
    assert max(args.ctx) < args.cache, "contexts must fit the cache"
    c = get_config(args.arch)

    if args.prefill_tokens:
        torch.manual_seed(3)
        n, hq, kh, hd = args.prefill_tokens, c.n_heads, c.n_kv_heads, c.head_dim
        q = torch.randn(n, hq, hd, device="cuda").bfloat16()
        k = torch.randn(n, kh, hd, device="cuda").bfloat16()
        v = torch.randn(n, kh, hd, device="cuda").bfloat16()
        for rep in range(2):
            for w in args.windows:
                ms = timed(lambda: ops.attn_prefill(q, k, v, window=w), 10, 2)
                print(f"prefill_attn n={n} hq={hq} kh={kh} hd={hd} window={w} "
                      f"rep={rep}: {ms:.3f} ms", flush=True)
        del q, k, v

    for kv in args.kv_dtypes.split(","):
        for w in args.windows:
            eng = LocalEngine({"name": "probe", "arch": args.arch,
                               "kv_dtype": kv, "sliding_window": w},
                              device="cuda:0")
            m = eng.model
            m.split_blocks = eng._pick_split_blocks()
            cache = eng._get_cache(args.cache)
            ws = m.new_decode_ws()
            ws.tok_long.fill_(42)
            for ctx in args.ctx:
                pos = torch.tensor([ctx], dtype=torch.int32, device="cuda")
                m.decode_step_ws(cache, pos, cache.max_seq, ws)
                g = torch.cuda.CUDAGraph()
                with torch.cuda.graph(g, stream=torch.cuda.Stream()):
                    m.decode_step_ws(cache, pos, cache.max_seq, ws)
                for rep in range(2):
                    print(f"decode_step arch={args.arch} kv={kv} window={w} "
                          f"ctx={ctx} cache={cache.max_seq} rep={rep}: "
                          f"{timed(g.replay, 100):.4f} ms/tok", flush=True)
                del g
            del eng, m, cache, ws
            torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
