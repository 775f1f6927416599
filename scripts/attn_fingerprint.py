"""Bitwise fingerprint of the attention kernels' outputs.

Prints one line per case with the SHA-256 of the bytes of every output of
the raw extension entry points (attn_fwd, attn_bwd_delta, attn_bwd,
attn_decode). Inputs come from a seeded CPU generator, so two builds of
the extension that do the same arithmetic in the same order print the
same lines; a refactor of the kernels must not change them.

The extension is imported from this script's own tree, so a second
checkout built elsewhere can be fingerprinted by running its copy.

Usage: python scripts/attn_fingerprint.py > fingerprint.txt
"""
import hashlib
import math
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch

import metis_amd._hip_ops as ext

HEAD_DIMS = (64, 80, 96, 128)


def digest(t):
    raw = t.detach().contiguous().cpu().view(torch.uint8).numpy().tobytes()
    return hashlib.sha256(raw).hexdigest()


def inputs(gen, *shapes):
    return [torch.randn(*s, generator=gen).to("cuda", torch.bfloat16)
            for s in shapes]


def main():
    gen = torch.Generator().manual_seed(1234)
    B = 2
    for D in HEAD_DIMS:
        scale = 1.0 / math.sqrt(D)
        for H, Hkv in ((4, 2), (6, 2)):
            for S in (128, 384):
                q, k, v, d_o = inputs(gen, (B, H, S, D), (B, Hkv, S, D),
                                      (B, Hkv, S, D), (B, H, S, D))
                o, lse = ext.attn_fwd(q, k, v, scale)
                delta = ext.attn_bwd_delta(o, d_o)
                dq, dk_h, dv_h = ext.attn_bwd(q, k, v, d_o, lse, delta, scale)
                outs = dict(o=o, lse=lse, delta=delta, dq=dq, dk_h=dk_h, dv_h=dv_h)
                print(f"attn D{D} H{H} Hkv{Hkv} S{S} "
                      + " ".join(f"{n}={digest(t)}" for n, t in outs.items()))
    for D in HEAD_DIMS:
        q, k, v = inputs(gen, (B, 4, 1, D), (B, 2, 300, D), (B, 2, 300, D))
        out = ext.attn_decode(q, k, v, 1.0 / math.sqrt(D))
        print(f"decode D{D} H4 Hkv2 S300 out={digest(out)}")


if __name__ == "__main__":
    main()
