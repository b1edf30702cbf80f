"""Diagnostic (not part of the product): decode-step attention over a packed layer
(rtkv_decode_attention_packed) against torch SDPA over the dense dequantized K'/V' the reference
keeps (modified_llama.py:140-142), on a cfg3-shaped layer (B = 1, S = 16384, Hkv = 32, D = 128 f16,
ratio 0.6, bits 2/4/8) and Llama-3-8B-shaped GQA (Hkv = 8).  Prints µs per step and the algorithmic
HBM bytes / time (packed codes + per-row scale/zp + kept_index / row_offset + labels gather).

--tail T[,T...]: after each no-tail line, the step over the packed rows followed by a dense tail of T
generated tokens (rtkv_decode_attention_packed_tail) next to dense SDPA over cat(K', tail), with the
rate of the added bytes 2·T·F·e / (t_T − t_0), t_0 the no-tail step.

--chunk T[,T...]: a multi-token step (rtkv_extend_attention_packed_tail) of T new tokens over the packed
rows and a tail of `older` + T rows, next to the same work done as T single-token steps of
rtkv_decode_attention_packed_tail (step t over the tail up to its own token), timed in the same run.
`older` takes the values of --tail (default 0,1024).

--gq: the layer is also kept in the rtkv-gq/1 format (group_quant=, n_outlier 4).  For the same layer, in this
process, in interleaved rounds (median and min..max over the rounds): the old gq kernel
(rtkv_gq_decode_attention), the gq step with a dense tail (rtkv_gq_decode_attention_tail) for each --tail
length (default 0,128,1024,4096), and the per-token step with the same tail
(rtkv_decode_attention_packed_tail) over the per-token codes of the same kept rows, beside the bytes
each format moves per row.

usage: decode_bench.py [cases e.g. 0,2] [iters] [--tail 0,128,1024,4096] [--chunk 1,4,16,64,256] [--gq]"""
import argparse
import os
import sys
import time

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "..", "realtime-kv-cache-compression_amd"))
sys.path.insert(0, os.path.join(HERE, "..", "tests", "golden"))
import rtkv  # noqa: E402
import synth  # noqa: E402


TD = {"float16": torch.float16, "bfloat16": torch.bfloat16}


def dev(stored, dtype):
    return torch.from_numpy(np.ascontiguousarray(stored, np.uint16).view(np.int16)).cuda().view(TD[dtype])


def timed(fn, iters):
    """µs per call: device events around `iters` calls after 10 warm-up calls."""
    for _ in range(10):
        fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / iters * 1e3


def run_tails(pk, k2, v2, n, q, Hkv, Hq, D, us0, tails, iters):
    """The step with a dense tail of T rows, for each T, against SDPA over cat(K', tail)."""
    F, e = Hkv * D, q.element_size()
    for T in tails:
        tail = rtkv.DecodeTail(1, F, q.dtype, "cuda", capacity=max(T, 1))
        if T:
            tail.append(torch.randn(1, T, F, device="cuda").to(q.dtype), torch.randn(1, T, F, device="cuda").to(q.dtype))
        us = timed(lambda: rtkv.decode_attention(pk, q, Hkv, tail=tail), iters)
        kd = torch.cat([k2[:, :n], tail.k[:, :T]], 1).view(1, n + T, Hkv, D).transpose(1, 2)
        vd = torch.cat([v2[:, :n], tail.v[:, :T]], 1).view(1, n + T, Hkv, D).transpose(1, 2)
        kd = kd.repeat_interleave(Hq // Hkv, 1).contiguous()
        vd = vd.repeat_interleave(Hq // Hkv, 1).contiguous()
        qq = q.view(1, Hq, 1, D)
        us_d = timed(lambda: torch.nn.functional.scaled_dot_product_attention(qq, kd, vd), iters)
        added = 2 * T * F * e
        rate = f"{added / (us - us0) / 1e3:.0f} GB/s" if T and us > us0 else "n/a"
        print(f"    tail T={T}: decode {us:.1f} us (no tail {us0:.1f} us; +{added/1e6:.2f} MB dense tail at {rate}) | "
              f"dense SDPA over cat(K', tail) {us_d:.1f} us", flush=True)


def run_chunks(pk, q1, Hkv, Hq, D, chunks, olders, iters):
    """One call of T new tokens against T single-token steps over the same layer and tail."""
    F = Hkv * D
    for older in olders:
        for T in chunks:
            n = older + T
            tk = torch.randn(1, n, F, device="cuda").to(q1.dtype)
            tv = torch.randn(1, n, F, device="cuda").to(q1.dtype)
            q = torch.randn(1, Hq, T, D, device="cuda").to(q1.dtype)
            whole = rtkv.DecodeTail.from_tensors(tk, tv, torch.tensor([n], device="cuda"))
            steps = [(q[:, :, t].contiguous(), rtkv.DecodeTail.from_tensors(tk, tv, torch.tensor([n - (T - 1 - t)], device="cuda")))
                     for t in range(T)]
            it = max(10, iters // max(1, T // 8))
            us = timed(lambda: rtkv.extend_attention(pk, q, Hkv, whole), iters)
            us_1 = timed(lambda: [rtkv.decode_attention(pk, qt, Hkv, tail=tl) for qt, tl in steps], it)
            print(f"    chunk T={T} older={older}: extend {us:.1f} us ({us / T:.1f} us/token) | {T} single steps {us_1:.1f} us "
                  f"({us_1 / T:.1f} us/token) | ratio {us_1 / us:.2f}x", flush=True)


def run_gq(S, Hkv, Hq, dtype="float16", D=128, ratio=0.6, iters=200, tails=(0, 128, 1024, 4096), rounds=5, n_outlier=4):
    """The gq step (old kernel, new entry point with each tail) and the per-token step on the same kept rows,
    interleaved: `rounds` rounds, each timing every variant for iters / rounds calls."""
    F, e = Hkv * D, 2
    K, V = synth.kv(11, 1, S, F, dtype)
    W = synth.attention_slice(11, 1, 8, S, rtkv.prompt_length(S), dtype)
    cfg = rtkv.CompressionConfig(num_hidden_layers=4, low_precision_bits=2, medium_precision_bits=4,
                                 high_precision_bits=8, early_layer_ratio=ratio, middle_layer_ratio=ratio,
                                 later_layer_ratio=ratio)
    comp = rtkv.RealTimePrefillCompressor(cfg, group_quant=rtkv.GroupQuantConfig(n_outlier=n_outlier))
    ids = torch.zeros(1, S, dtype=torch.long, device="cuda")
    k2, v2, info = comp.compress_layer_kv_cache(dev(K, dtype), dev(V, dtype), dev(W, dtype), ids, 1)
    pk, c = info["packed"], info["group_quant"]
    n = int(pk["rows"][0])
    q = torch.randn(1, Hq, D, device="cuda").to(TD[dtype])
    tl = {}
    for T in tails:
        tl[T] = rtkv.DecodeTail(1, F, q.dtype, "cuda", capacity=max(T, 1))
        if T:
            tl[T].append(torch.randn(1, T, F, device="cuda").to(q.dtype), torch.randn(1, T, F, device="cuda").to(q.dtype))
    variants = [("gq old kernel, no tail", lambda: c.attend(q))]
    variants += [(f"gq tail T={T}", (lambda t: lambda: c.attend(q, tail=t))(tl[T])) for T in tails]
    variants += [(f"per-token tail T={T}", (lambda t: lambda: rtkv.decode_attention(pk, q, Hkv, tail=t))(tl[T]))
                 for T in tails]
    us = {name: [] for name, _ in variants}
    for _ in range(rounds):
        for name, fn in variants:
            us[name].append(timed(fn, max(10, iters // rounds)))
    code = pk["codes_k"].numel() / max(n, 1)                        # mean code bytes per row and tensor
    gq_row, tok_row = code + 2 * Hkv * e + Hkv * n_outlier * e, code + 8
    print(f"S={S} Hkv={Hkv} Hq={Hq} {dtype} gq: kept {n}, n_outlier {n_outlier}; bytes per row and tensor: gq "
          f"{gq_row:.0f} (codes {code:.0f} + meta {2 * Hkv * e} + raw {Hkv * n_outlier * e}), per-token {tok_row:.0f}: "
          f"ratio {gq_row / tok_row:.3f}; {rounds} interleaved rounds of {max(10, iters // rounds)} calls", flush=True)
    med = {name: float(np.median(v)) for name, v in us.items()}
    for name, _ in variants:
        v = us[name]
        extra = ""
        if name.startswith("gq tail"):
            T = int(name.split("=")[1])
            extra = f" | over the empty tail {med[name] - med[f'gq tail T={tails[0]}']:+.1f} us" if T != tails[0] else \
                f" | old kernel / this {med['gq old kernel, no tail'] / med[name]:.2f}x"
            extra += f" | this / per-token step {med[name] / med[f'per-token tail T={T}']:.2f}x"
        print(f"    {name}: {med[name]:.1f} us (min {min(v):.1f}, max {max(v):.1f})" + extra, flush=True)


def run(S, Hkv, Hq, dtype="float16", D=128, ratio=0.6, iters=200, tails=(), chunks=()):
    F = Hkv * D
    K, V = synth.kv(11, 1, S, F, dtype)
    W = synth.attention_slice(11, 1, 8, S, rtkv.prompt_length(S), dtype)
    cfg = rtkv.CompressionConfig(num_hidden_layers=4, low_precision_bits=2, medium_precision_bits=4,
                                 high_precision_bits=8, early_layer_ratio=ratio, middle_layer_ratio=ratio,
                                 later_layer_ratio=ratio)
    comp = rtkv.RealTimePrefillCompressor(cfg)
    ids = torch.zeros(1, S, dtype=torch.long, device="cuda")
    k2, v2, info = comp.compress_layer_kv_cache(dev(K, dtype), dev(V, dtype), dev(W, dtype), ids, 1)
    pk = info["packed"]
    n = int(pk["rows"][0])
    q = torch.randn(1, Hq, D, device="cuda").to(TD[dtype])
    for _ in range(10):
        rtkv.decode_attention(pk, q, Hkv)
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters):
        rtkv.decode_attention(pk, q, Hkv)
    e1.record()
    torch.cuda.synchronize()
    us = e0.elapsed_time(e1) / iters * 1e3
    code_bytes = 2 * pk["codes_k"].numel()
    meta = n * (16 + 4 + 8 + 1)
    by = code_bytes + meta + q.numel() * 2 + Hq * D * 4
    # dense baseline: SDPA over the dequantized rows (GQA expanded as the reference's repeat_kv does)
    kd = k2[:, :n].view(1, n, Hkv, D).transpose(1, 2)
    vd = v2[:, :n].view(1, n, Hkv, D).transpose(1, 2)
    kd = kd.repeat_interleave(Hq // Hkv, 1).contiguous()
    vd = vd.repeat_interleave(Hq // Hkv, 1).contiguous()
    qq = q.view(1, Hq, 1, D)
    for _ in range(10):
        torch.nn.functional.scaled_dot_product_attention(qq, kd, vd)
    torch.cuda.synchronize()
    e0.record()
    for _ in range(iters):
        torch.nn.functional.scaled_dot_product_attention(qq, kd, vd)
    e1.record()
    torch.cuda.synchronize()
    us_d = e0.elapsed_time(e1) / iters * 1e3
    dense_by = 2 * n * Hq * D * 2
    print(f"S={S} Hkv={Hkv} Hq={Hq} {dtype}: kept {n}, packed {code_bytes/1e6:.2f} MB ({code_bytes*8/(2*n*F):.2f} bits/elem) "
          f"-> decode {us:.1f} us, {by/us/1e3:.0f} GB/s algorithmic | dense SDPA over K'/V' {us_d:.1f} us "
          f"({dense_by/1e6:.1f} MB, {dense_by/us_d/1e3:.0f} GB/s)", flush=True)
    if tails and not chunks:
        run_tails(pk, k2, v2, n, q, Hkv, Hq, D, us, tails, iters)
    if chunks:
        run_chunks(pk, q, Hkv, Hq, D, chunks, tails or (0, 1024), iters)


if __name__ == "__main__":
    rtkv.build()
    cases = ((16384, 32, 32), (32768, 32, 32), (16384, 8, 32), (131072, 8, 32), (131072, 8, 8), (32768, 32, 128),
             (32768, 32, 32, "bfloat16"), (131072, 8, 32, "bfloat16"))
    ap = argparse.ArgumentParser()
    ap.add_argument("cases", nargs="?", default=None, help="comma-separated case indices (default: all)")
    ap.add_argument("iters", nargs="?", type=int, default=200)
    ap.add_argument("--tail", default="", help="comma-separated dense tail lengths, e.g. 0,128,1024,4096")
    ap.add_argument("--chunk", default="", help="comma-separated numbers of new tokens per multi-token step, e.g. 1,4,16,64,256")
    ap.add_argument("--gq", action="store_true", help="the gq step (old kernel, new entry point with each tail) "
                                                      "against the per-token step on the same rows")
    args = ap.parse_args()
    only = [int(x) for x in args.cases.split(",")] if args.cases else range(len(cases))
    tails = tuple(int(x) for x in args.tail.split(",")) if args.tail else ()
    for i in only:
        if args.gq:
            run_gq(*cases[i], iters=args.iters, tails=tails or (0, 128, 1024, 4096))
            continue
        run(*cases[i], iters=args.iters, tails=tails, chunks=tuple(int(x) for x in args.chunk.split(",")) if args.chunk else ())
