"""Forward time of muse.CLIPTextEncoder against transformers' eager CLIP text model on the same GPU.

CLIP-L geometry (12 layers, width 768, 12 heads, 3072 intermediate, 77 tokens, vocabulary 49408), seeded random weights, batch 64 and 1,
bf16 and f32.  The two implementations alternate in one process: each is warmed up, then timed in rounds of device-event pairs around
blocks of iterations until about a second of GPU time per contender is filled; the median block gives the figure.  The fused causal
kernel's own time comes from ops.profile_start / profile_stop (its algorithmic work: 2 * 2 * B * heads * S^2 * head_dim flop).

    python scripts/clip_text_timing.py [--out profiles/clip_text_timing.json]
"""
import argparse
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "open-muse_amd"))

GEOM = dict(vocab_size=49408, hidden_size=768, intermediate_size=3072, num_hidden_layers=12, num_attention_heads=12,
            max_position_embeddings=77, projection_dim=768, hidden_act="quick_gelu", bos_token_id=49406, eos_token_id=49407, pad_token_id=49407)
SEQ = 77


def block_ms(fn, iters):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters):
        fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) / iters


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--seconds", type=float, default=1.0)
    args = ap.parse_args()
    import muse
    from muse import ops
    from transformers import CLIPTextConfig, CLIPTextModelWithProjection
    torch.manual_seed(0)
    hf = CLIPTextModelWithProjection(CLIPTextConfig(**GEOM)).eval()
    native = muse.CLIPTextEncoder.from_transformers(hf).to("cuda")
    results = []
    for dtype in (torch.bfloat16, torch.float32):
        eager = hf.to("cuda", dtype=dtype)
        native.set_compute_dtype(dtype)
        for batch in (64, 1):
            g = torch.Generator().manual_seed(batch)
            ids = torch.randint(0, 49406, (batch, SEQ), generator=g)
            ids[:, 0], ids[:, -1] = 49406, 49407
            ids = ids.cuda()
            with torch.no_grad():
                contenders = {"native": lambda: native(ids, return_dict=True, output_hidden_states=True),
                              "eager": lambda: eager(ids, return_dict=True, output_hidden_states=True)}
                once = {}
                for name, fn in contenders.items():       # warm-up: packing, first-use work, clocks
                    for _ in range(5):
                        fn()
                    torch.cuda.synchronize()
                    once[name] = block_ms(fn, 3)
                iters = {n: max(3, int(100.0 / once[n])) for n in contenders}      # ~0.1 s blocks
                rounds = max(3, int(round(args.seconds / 0.1)))
                samples = {n: [] for n in contenders}
                for _ in range(rounds):                                             # alternated
                    for name, fn in contenders.items():
                        samples[name].append(block_ms(fn, iters[name]))
                row = dict(dtype=str(dtype).replace("torch.", ""), batch=batch, seq=SEQ, rounds=rounds)
                for name in contenders:
                    row[f"{name}_ms"] = round(statistics.median(samples[name]), 4)
                    row[f"{name}_ms_min"] = round(min(samples[name]), 4)
                    row[f"{name}_ms_max"] = round(max(samples[name]), 4)
                row["eager_over_native"] = round(row["eager_ms"] / row["native_ms"], 3)
                if dtype == torch.bfloat16:
                    ops.profile_start()
                    for _ in range(20):
                        contenders["native"]()
                    rec = [(w, ms) for n, w, ms in ops.profile_stop() if n == "attn_causal_fwd_bf16"]
                    ms = statistics.median(m for _, m in rec)
                    row["causal_attn_us"] = round(ms * 1e3, 2)
                    row["causal_attn_tflops"] = round(rec[0][0] / (ms * 1e-3) / 1e12, 3)
            results.append(row)
            print(json.dumps(row), flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(dict(geometry=GEOM, device=torch.cuda.get_device_name(0), results=results), f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
