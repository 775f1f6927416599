"""CPU tests of the fp8 KV cache: the format (ops/kv8.py), the conformance
criterion's power on the kernel emulation and its mutants, the
dequantised fallback of decode_attention, and the kv_dtype="fp8" plumbing
of the ragged cache, ContinuousBatcher, generate_ragged and serve."""

import functools

import pytest
import torch

import decode_fp8_conformance as fc
from metis_amd.models.gpt import GPTModel, GPTModelSpec
from metis_amd.models.llama import LlamaModel, LLAMA_SPECS
from metis_amd.ops.attention import decode_attention
from metis_amd.ops.kv8 import kv_quant_store, quantize_kv_e4m3
from metis_amd.runtime.generate import (ContinuousBatcher, KVCache,
                                        RaggedKVCache, generate_ragged)

F8 = torch.float8_e4m3fn
B, H, HKV = 3, 8, 2
GPT_SPEC = GPTModelSpec("kv8-tiny", hidden_size=256, num_layers=2,
                        num_heads=4, vocab_size=512, seq_length=64)


# ---------------------------------------------------------------- format

def _round_trip_ratio(x):
    """max over rows of |x - x8 s| / (amax / 28), in float64."""
    x8, s = quantize_kv_e4m3(x)
    assert x8.dtype == F8 and x8.shape == x.shape
    assert s.dtype == torch.float32 and s.shape == x.shape[:-1]
    amax = x.double().abs().amax(dim=-1)
    err = (x.double() - x8.double() * s.double()[..., None]).abs().amax(dim=-1)
    return (err / (amax / 28)).max().item()


def test_round_trip_bound():
    """|x - x8 s| <= amax / 28: half a step of e4m3's top binade (16) times
    the scale amax / 448. The bound is exact arithmetic's. It is asserted
    on rows whose amax is 448 * 2^k, where the fp32 scale 2^k and every
    quotient are exact, so the definition computes exactly what the bound
    describes. On a general row the scale amax / 448 is itself rounded to
    fp32, and a bf16 element that sits exactly on a midpoint of the top
    binade then misses the bound by that rounding: measured 1.0000008 of
    the bound on the worst of 612 randn rows (printed, not asserted)."""
    g = torch.Generator().manual_seed(0)
    for gain in (1.0, 100.0, 1e-3):
        x = (torch.randn(4, 3, 17, 64, generator=g) * gain).to(torch.bfloat16)
        print(f"randn x {gain}: worst |x - x8 s| / (amax / 28) = "
              f"{_round_trip_ratio(x):.8f}")
    x = torch.randn(4, 3, 17, 64, generator=g)
    x = x / x.abs().amax(dim=-1, keepdim=True)          # |x| <= 1
    k = torch.randint(-8, 3, (4, 3, 17, 1), generator=g).float()
    x = (x * 448 * torch.exp2(k)).to(torch.bfloat16)    # amax = 448 * 2^k
    assert _round_trip_ratio(x) <= 1.0


def test_zero_row():
    x8, s = quantize_kv_e4m3(torch.zeros(2, 5, 64))
    assert (x8.view(torch.uint8) == 0).all()
    assert torch.isfinite(s).all() and (s > 0).all()


def test_midpoints_round_to_even():
    """amax = 448 makes the scale exactly 1; 17, 19, 21, 23 lie midway
    between the e4m3 neighbours 16, 18, 20, 22, 24 (step 2 in [16, 32))."""
    x = torch.zeros(1, 64)
    x[0, :5] = torch.tensor([448.0, 17.0, 19.0, 21.0, 23.0])
    x8, s = quantize_kv_e4m3(x)
    assert s.item() == 1.0
    assert x8.float()[0, :5].tolist() == [448.0, 16.0, 20.0, 20.0, 24.0]


# ------------------------------------------------- criterion and mutants

@functools.lru_cache(maxsize=None)
def _case(d, s, kind):
    ops = fc.fp8_input(B, H, HKV, s, d, kind)
    scale = fc.default_scale(d)
    return ops, scale, fc.reference(*ops, scale), fc.baseline(*ops, scale)


@pytest.mark.parametrize("kind", fc.KINDS)
@pytest.mark.parametrize("s", [5, 63, 65, 257])
@pytest.mark.parametrize("d", [64, 128])
def test_emulation_passes_and_mutants_fail(d, s, kind):
    ops, scale, ref, base = _case(d, s, kind)
    for ns in (1, 3):
        r = fc.ratio(fc.emulate(*ops, scale, num_splits=ns), base, ref)
        print(f"D={d} S={s} {kind} splits={ns}: emulation ratio {r:.3f}")
        assert r <= 1.0
    if s > 65:          # a single key out of 257 weighs too little
        return
    for mutant in fc.MUTANTS:
        if mutant == "tail_dropped" and s % fc.rows_per_step(d) == 0:
            continue
        r = fc.ratio(fc.emulate(*ops, scale, mutant=mutant), base, ref)
        print(f"D={d} S={s} {kind} {mutant}: ratio {r:.3g}")
        assert r > 1.0, mutant


def test_emulation_g8_geometry():
    """G = 8 takes other rows-in-flight / rows-per-rescale."""
    ops = fc.fp8_input(2, 8, 1, 65, 64, "row_scaled")
    scale = fc.default_scale(64)
    ref, base = fc.reference(*ops, scale), fc.baseline(*ops, scale)
    assert fc.ratio(fc.emulate(*ops, scale), base, ref) <= 1.0
    assert fc.ratio(fc.emulate(*ops, scale, mutant="wrong_kv_head"),
                    base, ref) <= 1.0      # Hkv = 1: the mutant is a no-op
    assert fc.ratio(fc.emulate(*ops, scale, mutant="last_key_dropped"),
                    base, ref) > 1.0


# ------------------------------------------------------------- fallback

@pytest.mark.parametrize("kind", fc.KINDS)
@pytest.mark.parametrize("d", [64, 128])
def test_fallback_meets_criterion_and_ignores_padding(d, kind):
    s = 65
    ops, scale, _, _ = _case(d, s, kind)
    q, k8, v8, ks, vs = ops
    lens = torch.tensor([65, 5, 33])
    ref = fc.reference(*ops, scale, lens=lens)
    base = fc.baseline(*ops, scale, lens=lens)
    # positions at or past each row's length, and the buffer's padding,
    # hold NaN bytes and NaN scales
    kp, vp, ksp, vsp = (t.clone() for t in fc.pad_cache(k8, v8, ks, vs, 96))
    for i, n in enumerate(lens.tolist()):
        kp.view(torch.uint8)[i, :, n:] = 0x7F
        vp.view(torch.uint8)[i, :, n:] = 0x7F
        ksp[i, :, n:] = float("nan")
        vsp[i, :, n:] = float("nan")
    got = decode_attention(q, kp[:, :, :80], vp[:, :, :80], kv_lens=lens,
                           k_scale=ksp[:, :, :80], v_scale=vsp[:, :, :80])
    assert got.shape == q.shape and got.dtype == q.dtype
    assert torch.isfinite(got).all()
    r = fc.ratio(got, base, ref)
    print(f"D={d} {kind}: fallback ratio {r:.3f}")
    assert r <= 1.0


def test_scales_need_lengths_and_each_other():
    q, k8, v8, ks, vs = fc.fp8_input(1, 2, 2, 4, 64, "randn")
    with pytest.raises(ValueError):
        decode_attention(q, k8, v8, k_scale=ks, v_scale=vs)
    with pytest.raises(ValueError):
        decode_attention(q, k8, v8, kv_lens=torch.tensor([4]), k_scale=ks)


# ------------------------------------------------------ store (eager path)

def test_store_eager_matches_definition_and_skips_out_of_range():
    g = torch.Generator().manual_seed(3)
    n, hkv, t, d, bsz, cap = 3, 2, 5, 64, 4, 12
    k = torch.randn(n, hkv, t, d, generator=g)
    v = torch.randn(n, hkv, t, d, generator=g)
    k8 = torch.full((bsz, hkv, cap, d), 0x55, dtype=torch.uint8).view(F8)
    v8 = k8.clone()
    ks = torch.full((bsz, hkv, cap), -7.0)
    vs = ks.clone()
    slots, pos = torch.tensor([2, 0, 3]), torch.tensor([0, 4, 9])
    kv_quant_store(k, v, k8, v8, ks, vs, slots, pos)
    ek8, eks = quantize_kv_e4m3(k)
    ev8, evs = quantize_kv_e4m3(v)
    written = torch.zeros(bsz, cap, dtype=torch.bool)
    for i in range(n):
        for j in range(t):
            p = int(pos[i]) + j
            if p >= cap:
                continue            # 9 + 3, 9 + 4: past the end, skipped
            sl = int(slots[i])
            written[sl, p] = True
            assert torch.equal(k8.view(torch.uint8)[sl, :, p],
                               ek8.view(torch.uint8)[i, :, j])
            assert torch.equal(v8.view(torch.uint8)[sl, :, p],
                               ev8.view(torch.uint8)[i, :, j])
            assert torch.equal(ks[sl, :, p], eks[i, :, j])
            assert torch.equal(vs[sl, :, p], evs[i, :, j])
    assert written.sum() == 5 + 5 + 3
    keep = ~written[:, None, :].expand(bsz, hkv, cap)
    assert (k8.view(torch.uint8)[keep] == 0x55).all()
    assert (v8.view(torch.uint8)[keep] == 0x55).all()
    assert (ks[keep] == -7.0).all() and (vs[keep] == -7.0).all()


# ------------------------------------------------------- runtime plumbing

def _model(family):
    torch.manual_seed(0)
    if family == "llama":
        spec = LLAMA_SPECS["llama-tiny"]
        model = LlamaModel(spec, dtype=torch.float32)
    else:
        spec = GPT_SPEC
        model = GPTModel(spec, dtype=torch.float32)
    model.eval()
    return model, spec


def _prompts(vocab, lens, seed=5):
    g = torch.Generator().manual_seed(seed)
    return [torch.randint(0, vocab, (n,), generator=g).tolist() for n in lens]


@pytest.mark.parametrize("family", ["llama", "gpt"])
def test_continuous_batcher_fp8_drains_and_reuses_slots(family):
    model, spec = _model(family)
    prompts = _prompts(spec.vocab_size, (5, 9, 3, 7))
    budgets = (6, 3, 8, 4)
    with torch.no_grad():
        cb = ContinuousBatcher(model, capacity=32, max_batch=2,
                               kv_dtype="fp8")
        rids = [cb.submit(p, n, temperature=0.0)
                for p, n in zip(prompts, budgets)]
        for _ in range(200):
            cb.step()
            for logits in cb._last_logits.values():
                assert torch.isfinite(logits).all()
            if cb.active == 0 and not cb._pending:
                break
    assert cb.active == 0 and not cb._pending
    for rid, p, n in zip(rids, prompts, budgets):
        assert len(cb.finished[rid]) == len(p) + n
        assert cb.finished[rid][:len(p)] == p
    k8, v8, ks, vs = cb.cache._kv[0]
    assert k8.dtype == F8 and v8.dtype == F8
    assert ks.dtype == torch.float32 and ks.shape == k8.shape[:-1]
    assert cb.cache.kv_dtype == "fp8"


def test_retired_slot_is_overwritten_by_the_next_prefill():
    model, spec = _model("llama")
    first, second = _prompts(spec.vocab_size, (9, 6), seed=8)
    with torch.no_grad():
        cb = ContinuousBatcher(model, capacity=32, max_batch=1,
                               kv_dtype="fp8")
        cb.submit(first, 3, temperature=0.0)
        rid2 = cb.submit(second, 2, temperature=0.0)
        while not cb.finished:
            cb.step()
        old = [tuple(t.clone() for t in cb.cache._kv[i])
               for i in range(spec.num_layers)]
        cb._admit()                     # the second request takes slot 0
        assert cb._slots[0]["rid"] == rid2
        pre = KVCache()
        model(torch.tensor([second]), cache=pre, pos_offset=0)
    n = len(second)
    for i in range(spec.num_layers):
        k8, v8, ks, vs = cb.cache._kv[i]
        ek8, eks = quantize_kv_e4m3(pre._kv[i][0])
        ev8, evs = quantize_kv_e4m3(pre._kv[i][1])
        assert torch.equal(ks[0, :, :n], eks[0]) and torch.equal(vs[0, :, :n], evs[0])
        assert torch.equal(k8.view(torch.uint8)[0, :, :n],
                           ek8.view(torch.uint8)[0])
        assert torch.equal(v8.view(torch.uint8)[0, :, :n],
                           ev8.view(torch.uint8)[0])
        assert not torch.equal(ks[0, :, :n], old[i][2][0, :, :n])
        # what lies past the new prompt is the old request's, untouched
        assert torch.equal(ks[0, :, n:], old[i][2][0, :, n:])


def test_fp8_cache_tracks_the_bf16_cache():
    """Same model, same prompts: per-step logits of the quantised cache
    stay close to the exact cache's (fp32 model, so the difference is the
    quantisation alone). e4m3 keeps 3 mantissa bits: K and V carry up to
    2^-4 relative error per element; logits of these tiny models are
    O(1), and a broken scale hand-over shows as O(1) differences."""
    model, spec = _model("llama")
    prompts = _prompts(spec.vocab_size, (5, 9, 3))
    nxt = torch.tensor([[7], [11], [13]])
    out = {}
    with torch.no_grad():
        caches = []
        for p in prompts:
            c = KVCache()
            model(torch.tensor([p]), cache=c, pos_offset=0)
            caches.append(c)
        for kv_dtype in ("bf16", "fp8"):
            cache = RaggedKVCache.from_prefills(
                caches, [len(p) for p in prompts], 4, kv_dtype=kv_dtype)
            out[kv_dtype] = model(nxt, cache=cache,
                                  pos_offset=cache.lengths.clone())[:, -1]
    diff = (out["fp8"] - out["bf16"]).abs().max().item()
    spread = out["bf16"].abs().max().item()
    print(f"fp8 vs exact cache: max logit diff {diff:.4g} of {spread:.4g}")
    assert torch.isfinite(out["fp8"]).all()
    assert diff <= 0.125 * spread


def test_generate_ragged_fp8():
    model, spec = _model("gpt")
    prompts = _prompts(spec.vocab_size, (4, 7, 2))
    outs = generate_ragged(model, prompts, 5, temperature=0.0,
                           kv_dtype="fp8")
    for p, o in zip(prompts, outs):
        assert o[:len(p)] == p and len(o) == len(p) + 5
    with pytest.raises(AssertionError):
        generate_ragged(model, prompts, 1, kv_dtype="int4")


def test_bf16_cache_has_no_scales():
    cache = RaggedKVCache(torch.tensor([1, 2]))
    assert cache.kv_dtype == "bf16" and cache.kv_scales(0) is None


# ----------------------------------------------------------------- serve

def test_serve_rejects_fp8_cache_without_continuous(capsys):
    from metis_amd.cli import serve

    with pytest.raises(SystemExit):
        serve.parse_args(["--kv-dtype", "fp8"])
    assert "--continuous" in capsys.readouterr().err
    args = serve.parse_args(["--kv-dtype", "fp8", "--continuous"])
    assert args.kv_dtype == "fp8"
    assert serve.parse_args([]).kv_dtype == "bf16"
    model, spec = _model("gpt")
    with pytest.raises(ValueError):
        serve.build_app(model, spec, continuous=False, kv_dtype="fp8")


def test_serve_health_reports_kv_dtype_and_answers():
    from fastapi.testclient import TestClient

    from metis_amd.cli import serve

    model, spec = _model("gpt")
    client = TestClient(serve.build_app(model, spec, continuous=True,
                                        max_batch=2, kv_dtype="fp8"))
    assert client.get("/health").json()["kv_dtype"] == "fp8"
    prompts = _prompts(spec.vocab_size, (4, 6))
    r = client.post("/generate", json={"tokens": prompts,
                                       "max_new_tokens": 3})
    assert r.status_code == 200
    for p, o in zip(prompts, r.json()["tokens"]):
        assert o[:len(p)] == p and len(o) == len(p) + 3
    plain = TestClient(serve.build_app(model, spec))
    assert plain.get("/health").json()["kv_dtype"] == "bf16"
