"""Measures the warm-start path on the GPU (needs one; no fallback):
(a) VAE encode time at batch 8 next to the VAE decoder's forward time, same run, device events over windows of about 0.6 s, alternating;
(b) wall time of whole pipeline calls of the headline workload (MusicLDM + DPS inpainting, 10 s clips, batch 8, 200-step schedule,
    latents out) at strength 1.0 (no init: the cold path) and 0.5 (`init_audio` = the measurement), alternating, host clock around a
    device synchronise.  Expectation to confirm or refute: warm = n_run / N of cold + one encode.

    python scripts/dev/warm_start_bench.py --out profiles/warm_start.json [--steps 200] [--repeats 2]"""
import argparse
import json
import os
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))


def event_ms(fn, warmup, iters):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(iters):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / iters


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--batch", type=int, default=8)
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--repeats", type=int, default=2)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "needs a GPU"
    import bench
    B = args.batch
    device = torch.device("cuda")
    pipe, op, measurement, latents, cond, L = bench.build_problem(B, 0, device)
    enc, vae = pipe.vae_encoder, pipe.vae
    mel = (2.0 * torch.randn(B, 1000, 64, generator=torch.Generator().manual_seed(0)) - 4.0).to(device)
    z = torch.randn(B, 8, 250, 16, generator=torch.Generator().manual_seed(1)).to(device)
    enc_ms, dec_ms = [], []
    for _ in range(3):                                        # alternate the two so that drift hits both
        enc_ms.append(event_ms(lambda: enc.encode_hip(mel), 3, 150))
        dec_ms.append(event_ms(lambda: vae.decode_hip(z, 1.0, keep_state=False), 3, 100))
    res = {"batch": B, "encode_ms": [round(v, 3) for v in enc_ms], "decode_fwd_ms": [round(v, 3) for v in dec_ms],
           "encode_over_decode": round(min(enc_ms) / min(dec_ms), 3)}
    pe = cond["class_labels"][:B]
    kw = dict(prompt_embeds=pe, audio_length_in_s=10.0, num_inference_steps=args.steps, measurement=measurement, show_progress=False,
              output_type="latent", eta=pipe._bench["eta"], ip_guidance_rate=pipe._bench["rate"], guidance_scale=pipe._bench["gscale"])
    pipe.assume_uncond_equals_cond = True

    def call(**extra):
        gens = [torch.Generator().manual_seed(k) for k in range(B)]
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        pipe(generator=gens, **dict(kw, **extra))
        torch.cuda.synchronize()
        return time.perf_counter() - t0, len(pipe.last_losses)
    call(num_inference_steps=4)                               # warm-up: every shape of the timed calls
    call(num_inference_steps=4, init_audio=measurement, strength=0.5)
    cold, warm = [], []
    for _ in range(args.repeats):
        c, nc = call()
        w, nw = call(init_audio=measurement, strength=0.5)
        cold.append(round(c, 4))
        warm.append(round(w, 4))
    res.update({"steps": args.steps, "cold_wall_s": cold, "cold_steps": nc, "warm_strength": 0.5, "warm_wall_s": warm, "warm_steps": nw,
                "warm_over_cold": round(min(warm) / min(cold), 4),
                "expected_warm_s": round(min(cold) * nw / nc + min(enc_ms) / 1e3, 4)})
    line = json.dumps(res)
    print(line)
    if args.out:
        with open(args.out, "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
