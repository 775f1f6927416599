"""Weight-only fp8 quantisation of a model for the decode/serving path.

quantize_for_decode() swaps every block linear and the LM head of a
tp = pp = 1 GPTModel / LlamaModel for ops.w8.W8Linear (e4m3fn weights,
per-channel fp32 scales), in place; the bf16 weights are dropped with the
modules that held them. Embeddings and norms keep their dtype.

The models need no change: their cache (serving) branches and the plain
forward call the linears as modules. The only code that reads ``.weight``
of a linear directly is the sequence-parallel branch (tp > 1 only) and the
METIS_FC1_EPILOGUE=1 fused-MLP branch; both are refused here.
"""

from __future__ import annotations

import os

import torch.nn as nn

from metis_amd.models.gpt import GPTModel
from metis_amd.models.llama import LlamaModel
from metis_amd.ops.w8 import W8Linear

_GPT_LINEARS = ("qkv", "proj", "fc1", "fc2")
_LLAMA_LINEARS = ("qkv", "proj", "gate_up", "down")


def weight_dtype_of(model: nn.Module) -> str:
    """'fp8' for a model quantised by quantize_for_decode, else 'bf16'
    (the serving CLI's names)."""
    return getattr(model, "weight_dtype", "bf16")


def quantize_for_decode(model: nn.Module) -> nn.Module:
    if isinstance(model, LlamaModel):
        names = _LLAMA_LINEARS
    elif isinstance(model, GPTModel):
        names = _GPT_LINEARS
    else:
        raise TypeError(
            f"quantize_for_decode supports GPTModel and LlamaModel, not "
            f"{type(model).__name__} (MoE experts are out of scope)")
    if model.tp != 1 or getattr(model, "sp", False):
        raise ValueError("quantize_for_decode needs tp = 1: W8Linear has no "
                         "tensor-parallel collectives around it")
    if not (model.has_embedding and model.has_head):
        raise ValueError("quantize_for_decode needs the whole model (pp = 1)")
    if model.training:
        raise ValueError("quantize_for_decode is inference-only: call "
                         "model.eval() first")
    if (os.environ.get("METIS_FC1_EPILOGUE") == "1"
            or any(getattr(b, "_lt_mlp", False) for b in model.blocks)):
        raise ValueError("METIS_FC1_EPILOGUE=1 reads fc1/fc2 weights "
                         "directly; unset it to serve fp8 weights")
    if getattr(model, "weight_dtype", None) == "fp8":
        return model

    for block in model.blocks:
        for name in names:
            setattr(block, name, W8Linear.from_linear(getattr(block, name)))
    model.head = W8Linear.from_linear(model.head)
    model.weight_dtype = "fp8"
    return model
