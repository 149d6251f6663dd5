"""CPU reference (torch_ref, fp32): fp8-KV against bf16-KV logits gap and
greedy-token agreement over 64 decode steps on random-init models. Figures
in profiles/r04_fp8_kv.md."""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

from adversarial_spec_amd.models import LlamaModel, get_config  # noqa: E402
from adversarial_spec_amd.models.config import LlamaConfig  # noqa: E402

GPU_TINY = LlamaConfig(name="gpu-tiny", dim=512, n_layers=3, n_heads=4, n_kv_heads=2,
    ffn_dim=1024, vocab_size=1024, max_seq_len=2048, rope_theta=10000.0)
def cos(a,b): return torch.nn.functional.cosine_similarity(a[None].float(), b[None].float()).item()
for name, cfg in (("gpu-tiny(hd128)", GPU_TINY), ("tiny(hd32)", get_config("tiny"))):
    m = LlamaModel(cfg, device="cpu", seed=9).init_random()
    prompt = torch.arange(1, 200)
    cb, c8 = m.new_cache(512), m.new_cache(512, kv_dtype="fp8")
    lb, l8 = m.prefill(prompt, cb), m.prefill(prompt, c8)
    # free-running greedy on each cache
    tb, t8 = [], []
    for _ in range(64):
        tb.append(int(lb.argmax())); lb = m.decode_one(tb[-1], cb)
    for _ in range(64):
        t8.append(int(l8.argmax())); l8 = m.decode_one(t8[-1], c8)
    agree = sum(a == b for a, b in zip(tb, t8))
    div = next((i for i,(a,b) in enumerate(zip(tb,t8)) if a!=b), None)
    # teacher-forced on the bf16 tokens: per-step logits gap
    cb, c8 = m.new_cache(512), m.new_cache(512, kv_dtype="fp8")
    lb, l8 = m.prefill(prompt, cb), m.prefill(prompt, c8)
    gaps, top1 = [], 0
    for tok in tb:
        lb, l8 = m.decode_one(tok, cb), m.decode_one(tok, c8)
        gaps.append(1 - cos(lb, l8)); top1 += int(lb.argmax() == l8.argmax())
    rel = ((lb - l8).abs().max() / lb.abs().max()).item()
    print(f"{name}: free-running greedy agreement {agree}/64 (first divergence {div}); "
          f"teacher-forced: top-1 agreement {top1}/64, 1-cos mean {sum(gaps)/64:.3e} max {max(gaps):.3e}, "
          f"last-step max|dlogit|/max|logit| {rel:.3e}")
