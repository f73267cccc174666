"""Per-crystal key counts in the fp32 training path (DosxAttn.key_ptr / DosxFfn.att_key_ptr / DosxFfnBwd.att_key_ptr,
Trainer(per_crystal_keys=True)): a batch of B crystals computes - forward AND backward - what B batch-size-1 passes compute,
the setting the reference trains the phonon model and evaluates both models in (main_phDOS.py:52-55, main_eDOS.py:55-56).

Kernel level: ops.attention_fwd / attention_bwd against gpu_util._attn_ref in float64, run per query crystal over its keys [0, n)
only, with test_gpu_attention._attention_case's bounds.  Encoder level: functional.encoder_fwd / encoder_bwd against the float64
oracle's transformer_encoder run crystal by crystal, with test_gpu_ffn's tolerances.  Model level: Trainer.forward_backward against
the oracle's B batch-1 forwards and the autograd gradient of its loss through them."""
import functools
import math

import pytest
import torch

from tests.gpu_util import DEV, _attn_ref, err, ops, rnd

pytestmark = pytest.mark.gpu

# (Sq, Bq, Nk, Bk, H, counts)
CASES = {
    "nk12": (17, 4, 12, 2, 64, (1, 12)),                  # <= 16 keys, Bq = 2 Bk
    "nk37": (51, 6, 37, 3, 128, (16, 17, 37)),            # both sides of a 16-key tile edge
    "nk64_h256": (33, 3, 64, 3, 256, (1, 33, 64)),        # H 256: the partial-dK/dV dq kernel not LDS-resident
    "nk130": (5, 2, 130, 2, 64, (3, 129)),                # streamed, NJ 13, key group 2
    "nk320": (9, 2, 320, 2, 128, (209, 320)),             # last fused key count
    "nk330": (5, 4, 330, 2, 64, (5, 330)),                # general kernels
    "nk400_h256": (3, 2, 400, 2, 256, (321, 17)),         # general kernels, H 256
}
DROP = 0.35
OUT_TOL, GRAD_TOL = 3e-5, 5e-5      # test_gpu_attention._attention_case: out / probs, and stats / dx / dkvhat / dgamma0 / dbeta0


def _forms():
    """(case, aligned, pkv, one_launch): pkv / one-launch / aligned only where _attention_case applies them (<= 64 keys)."""
    out = []
    for name, c in CASES.items():
        if c[2] <= 64:
            for aligned in (False, True):
                out += [(name, aligned, False, False), (name, aligned, True, False), (name, aligned, True, True)]
        else:
            out.append((name, False, False, False))
    return out


FORMS = _forms()
FORM_IDS = [f"{n}-{'al' if al else 'st'}-{'pkv' if p else 'dkv'}{'-one' if o else ''}" for n, al, p, o in FORMS]


def _inputs(name, drop):
    Sq, Bq, Nk, Bk, H, _ = CASES[name]
    x = rnd(Sq * Bq, H, seed=1)
    kv = rnd(Nk * Bk, H, seed=2)            # the rows past a crystal's count hold random numbers, not zeros
    gam, bet = rnd(H, seed=3), 0.3 * rnd(H, seed=4)
    dout = rnd(Sq * Bq, H, seed=5)
    mask = None
    if drop:
        mask = (torch.rand(Bq, Sq, Nk, generator=torch.Generator().manual_seed(9)) >= DROP).float().to(DEV) / (1 - DROP)
    return x, kv, gam, bet, dout, mask


@functools.lru_cache(maxsize=None)
def _reference(name, counts, drop):
    """float64: every query crystal bq on its own, over the keys [0, n) of key crystal bq % Bk (n = 0: out = x)."""
    Sq, Bq, Nk, Bk, H, _ = CASES[name]
    x, kv, gam, bet, dout, mask = _inputs(name, drop)
    x, kv, gam, bet = (t.double().requires_grad_(True) for t in (x, kv, gam, bet))
    kv3 = kv.reshape(Nk, Bk, H)
    out = [None] * Bq
    probs = torch.zeros(Bq, Sq, Nk, dtype=torch.float64, device=DEV)
    for bq in range(Bq):
        n = min(max(counts[bq % Bk], 0), Nk)
        xq = x.reshape(Sq, Bq, H)[:, bq]
        if n == 0:
            out[bq] = xq
            continue
        m = None if mask is None else mask[bq:bq + 1, :, :n].double()
        o, p = _attn_ref(xq, kv3[:n, bq % Bk].reshape(n, H), gam, bet, Sq, 1, n, 1, H, 1, 0, m)
        out[bq] = o
        probs[bq, :, :n] = p[0].detach()
    out = torch.stack(out, 1).reshape(Sq * Bq, H)
    out.backward(dout.double())
    o = out.detach()
    return dict(out=o, probs=probs, mean=o.mean(1), rstd=1 / torch.sqrt(o.var(1, unbiased=False) + 1e-5),
                dx=x.grad, dkv=kv.grad, dg=gam.grad, db=bet.grad)


def _run(name, counts, drop, aligned=True, pkv=False, one_launch=False, accumulate=False, poison=False, fwd_only=False):
    """One forward + backward on the GPU.  counts None: key_ptr NULL.  poison: NaN in the kvhat rows and mask entries at key index
    >= n.  Every output buffer starts as NaN (dkvhat: as 0.5 when accumulating)."""
    from dostransformer_amd import _lib
    from dostransformer_amd._lib import Attn
    Sq, Bq, Nk, Bk, H, _ = CASES[name]
    lib = _lib.load()
    o = ops()
    x, kv, gam, bet, dout, mask = _inputs(name, drop)
    kp = None
    if counts is not None:
        kp = torch.tensor([0] + list(torch.tensor(counts).cumsum(0)), dtype=torch.int32, device=DEV)
        if poison:
            kv3 = kv.reshape(Nk, Bk, H)
            for bk in range(Bk):
                kv3[min(max(counts[bk], 0), Nk):, bk] = float("nan")
            if mask is not None:
                for bq in range(Bq):
                    mask[bq, :, min(max(counts[bq % Bk], 0), Nk):] = float("nan")
    nan = lambda *s: torch.full(s, float("nan"), device=DEV)
    a = Attn()
    a.Sq, a.Bq, a.Nk, a.Bk, a.H, a.q_stride_s, a.q_stride_b = Sq, Bq, Nk, Bk, H, Bq, 1
    out, probs, qstats, ostats = nan(Sq * Bq, H), nan(Bq, Sq, Nk), nan(Sq * Bq, 2), nan(Sq * Bq, 2)
    a.x, a.kvhat, a.gamma0, a.beta0 = x.data_ptr(), kv.data_ptr(), gam.data_ptr(), bet.data_ptr()
    a.out, a.probs, a.qstats, a.out_stats = out.data_ptr(), probs.data_ptr(), qstats.data_ptr(), ostats.data_ptr()
    a.drop_mask = mask.data_ptr() if mask is not None else None
    a.key_ptr = kp.data_ptr() if kp is not None else None
    pkv_path = pkv and bool(lib.dosx_attention_pkv_supported(Nk, H))
    prev = lib.dosx_attention_aligned_mode(-1 if aligned else 0)
    try:
        o.attention_fwd(a)
        res = dict(out=out, probs=probs, ostats=ostats)
        if fwd_only:
            torch.cuda.synchronize()
            return res
        dx, dsc = nan(Sq * Bq, H), nan(Bq, Sq, Nk)
        dkv = torch.full((Nk * Bk, H), 0.5, device=DEV) if accumulate else nan(Nk * Bk, H)
        nqt, nkt = (Sq + 31) // 32, ((Nk + 15) // 16 if pkv_path else (Nk + 31) // 32)
        part = nan(Bq * nqt + Bk * nkt, 2 * H)
        a.dout, a.dx, a.dscores, a.dkvhat, a.dkv_accumulate = dout.data_ptr(), dx.data_ptr(), dsc.data_ptr(), dkv.data_ptr(), int(accumulate)
        a.partials_q = part.data_ptr()
        a.partials_kv = part.data_ptr() + 4 * Bq * nqt * 2 * H
        if pkv:
            kvp = nan(Bq * nqt * Nk, H)
            a.dkv_part = kvp.data_ptr()
        if pkv_path:
            a.dscores = None
            if one_launch:
                a.dkv_cnt = o.COUNTERS.take(DEV, Bk)
        o.attention_bwd(a)
        torch.cuda.synchronize()
    finally:
        lib.dosx_attention_aligned_mode(prev)
    res.update(dx=dx, dkv=dkv, part=part, part_kv=part[Bq * nqt:], dsc=None if pkv_path else dsc)
    return res


def _check(name, counts, drop, got, accumulate):
    Sq, Bq, Nk, Bk, H, _ = CASES[name]
    ref = _reference(name, tuple(counts), drop)
    figs = dict(out=err(got["out"], ref["out"]), probs=err(got["probs"], ref["probs"]),
                mean=err(got["ostats"][:, 0], ref["mean"]), rstd=err(got["ostats"][:, 1], ref["rstd"]),
                dx=err(got["dx"], ref["dx"]))
    dkv = got["dkv"] - 0.5 if accumulate else got["dkv"]
    ps = got["part"].double().sum(0)
    figs.update(dkv=err(dkv, ref["dkv"]), dg=err(ps[:H], ref["dg"]), db=err(ps[H:], ref["db"]))
    print(name, counts, "drop" if drop else "nodrop", {k: f"{v:.2e}" for k, v in figs.items()})
    for k in ("out", "probs"):
        assert figs[k] < OUT_TOL, (k, figs[k])
    for k in ("mean", "rstd", "dx", "dkv", "dg", "db"):
        assert figs[k] < GRAD_TOL, (k, figs[k])
    # the contract's zeros: probs (and dscores, when the form writes them) past n; dkvhat rows past n are 0.0 when not
    # accumulating and left alone when accumulating
    dkv3 = got["dkv"].reshape(Nk, Bk, H)
    for bq in range(Bq):
        n = min(max(counts[bq % Bk], 0), Nk)
        assert bool((got["probs"][bq, :, n:] == 0).all())
        if got["dsc"] is not None:
            assert bool((got["dsc"][bq, :, n:] == 0).all())
    for bk in range(Bk):
        n = min(max(counts[bk], 0), Nk)
        assert bool((dkv3[n:, bk] == (0.5 if accumulate else 0.0)).all())


@pytest.mark.parametrize("drop", [False, True], ids=["nodrop", "drop"])
@pytest.mark.parametrize("accumulate", [False, True], ids=["fresh", "acc"])
@pytest.mark.parametrize("form", FORMS, ids=FORM_IDS)
def test_attention_fwd_bwd_over_own_keys(form, accumulate, drop):
    name, aligned, pkv, one = form
    counts = CASES[name][5]
    got = _run(name, counts, drop, aligned, pkv, one, accumulate)
    _check(name, counts, drop, got, accumulate)


def _same(u, v, what):
    for k in u:
        if u[k] is None or k == "part_kv":
            continue
        assert not torch.isnan(v[k]).any(), (what, k)
        assert torch.equal(u[k], v[k]), (what, k)


@pytest.mark.parametrize("drop", [False, True], ids=["nodrop", "drop"])
@pytest.mark.parametrize("form", FORMS, ids=FORM_IDS)
def test_nothing_past_the_count_is_read(form, drop):
    """NaN in the kvhat rows >= n and in the mask entries >= n, every output buffer prefilled with NaN: bitwise the run on the
    clean inputs, no NaN in any output; a second run is bitwise equal (fixed reduction orders)."""
    name, aligned, pkv, one = form
    counts = CASES[name][5]
    clean = _run(name, counts, drop, aligned, pkv, one)
    dirty = _run(name, counts, drop, aligned, pkv, one, poison=True)
    _same(clean, dirty, "poisoned")
    _same(clean, _run(name, counts, drop, aligned, pkv, one), "second run")
    # the key-side partial rows of key tiles past n are zeros: the sink's column sums need no mask
    Sq, Bq, Nk, Bk, H, _ = CASES[name]
    pk = dirty["part_kv"]
    tile = 16 if (pkv and Nk <= 64) else 32
    rows = pk.shape[0] // Bk
    for bk in range(Bk):
        for t in range(rows):
            if t * tile >= counts[bk]:
                assert bool((pk[bk * rows + t] == 0).all()), (bk, t)


@pytest.mark.parametrize("drop", [False, True], ids=["nodrop", "drop"])
@pytest.mark.parametrize("form", FORMS, ids=FORM_IDS)
def test_full_counts_are_bitwise_no_key_ptr(form, drop):
    """counts = [Nk] * Bk gives bitwise what key_ptr = NULL gives, for every output; a count above Nk is clamped to Nk."""
    name, aligned, pkv, one = form
    Sq, Bq, Nk, Bk, H, _ = CASES[name]
    base = _run(name, None, drop, aligned, pkv, one, accumulate=True)
    _same(base, _run(name, [Nk] * Bk, drop, aligned, pkv, one, accumulate=True), "full counts")
    _same(base, _run(name, [Nk + 7] * Bk, drop, aligned, pkv, one, accumulate=True), "clamped counts")


@pytest.mark.parametrize("drop", [False, True], ids=["nodrop", "drop"])
@pytest.mark.parametrize("form", FORMS, ids=FORM_IDS)
def test_a_crystal_without_keys_passes_through(form, drop):
    """n = 0: out == x bitwise, zero probabilities, dx == dout (the residual alone), zero key gradients, nothing divides by zero."""
    name, aligned, pkv, one = form
    Sq, Bq, Nk, Bk, H, counts = CASES[name]
    counts = [0] + list(counts[1:])
    got = _run(name, counts, drop, aligned, pkv, one, poison=True)
    x, _, _, _, dout, _ = _inputs(name, drop)
    for k, v in got.items():
        if v is not None:
            assert not torch.isnan(v).any(), k
    for bq in range(0, Bq, Bk):
        assert torch.equal(got["out"].reshape(Sq, Bq, H)[:, bq], x.reshape(Sq, Bq, H)[:, bq])
        assert torch.equal(got["dx"].reshape(Sq, Bq, H)[:, bq], dout.reshape(Sq, Bq, H)[:, bq])
        assert bool((got["probs"][bq] == 0).all())
    assert bool((got["dkv"].reshape(Nk, Bk, H)[:, 0] == 0).all())
    _check(name, counts, drop, got, False)


# ------------------------------------------------------------------------------------------------------------------
# encoder level
# ------------------------------------------------------------------------------------------------------------------
ENC_SHAPES = {
    "nk16_h64": (51, 4, 64, 2, (1, 2, 12, 16), 16),       # the <= 16-key prologue and the aligned epilogue
    "nk37_h128": (51, 4, 128, 2, (2, 17, 33, 37), 37),    # aligned forward, fused backward
    "nk37_h64": (51, 4, 64, 2, (2, 17, 33, 37), 37),      # ... and, with a switch off, the separate launches
}


def _enc_params(H, T, seed):
    g = torch.Generator().manual_seed(seed)
    r = lambda *s, scale=1.0: (torch.randn(*s, generator=g, dtype=torch.float64) * scale).float().to(DEV)
    P = {}
    for t in range(T):
        lp = f"enc.layers.{t}"
        P[lp + ".fc1.weight"], P[lp + ".fc1.bias"] = r(4 * H, H, scale=H ** -0.5), r(4 * H, scale=0.1)
        P[lp + ".fc2.weight"], P[lp + ".fc2.bias"] = r(H, 4 * H, scale=(4 * H) ** -0.5), r(H, scale=0.1)
        for k in (0, 1):
            P[lp + f".layer_norms.{k}.weight"], P[lp + f".layer_norms.{k}.bias"] = 1 + r(H, scale=0.1), r(H, scale=0.1)
    P["enc.layer_norm.weight"], P["enc.layer_norm.bias"] = 1 + r(H, scale=0.1), r(H, scale=0.1)
    return P


def _encoder_case(shape, drop, off=None):          # off: the switch the caller has turned off around this call (printed)
    from oracle import dos_oracle as O
    from dostransformer_amd import functional as Fn
    Sq, B, H, T, counts, Nk = ENC_SHAPES[shape]
    o = ops()
    P = _enc_params(H, T, 11)
    G = {k: torch.zeros_like(v) for k, v in P.items()}
    x = rnd(Sq * B, H, seed=21)
    kv = rnd(Nk, B, H, seed=22)                           # rows past a crystal's count: random numbers
    kp = torch.tensor([0] + list(torch.tensor(counts).cumsum(0)), dtype=torch.int32, device=DEV)
    # the key rows as the program hands them over: pre-normalised (the parameter-free part of LayerNorm-0), row j * B + b
    kvl = kv.double().requires_grad_(True)
    kvn = torch.nn.functional.layer_norm(kvl, (H,))
    kvhat = kvn.detach().float().reshape(Nk * B, H).contiguous()
    seed = torch.tensor([1234567], dtype=torch.int64, device=DEV)
    Fn.DROP_MASK_LOG = []
    try:
        y, ctx = Fn.encoder_fwd(P, "enc", x, Sq, B, B, 1, kvhat, Nk, B, H, T, drop=(0.25, seed, 0) if drop else None, key_ptr=kp)
        masks = [m.clone() for _, _, m in Fn.DROP_MASK_LOG]
    finally:
        Fn.DROP_MASK_LOG = None
    w = rnd(Sq * B, H, seed=23)
    dkv = torch.zeros(Nk * B, H, device=DEV)
    sink = o.GradSink(torch.device(DEV))
    dx = Fn.encoder_bwd(P, G, "enc", ctx, w.clone(), dkv, sink)
    sink.flush()
    sink.release()
    torch.cuda.synchronize()
    kvn.backward(dkv.double().reshape(Nk, B, H))          # the key normalisation's backward: dkvhat -> gradient of the raw keys
    dkv_raw = kvl.grad
    # oracle: crystal by crystal over its own (raw) keys
    p64 = {k.replace("enc.", "e.", 1): v.detach().double().cpu().requires_grad_(True) for k, v in P.items()}
    x64 = x.double().cpu().reshape(Sq, B, H).requires_grad_(True)
    kv64 = kv.double().cpu().requires_grad_(True)
    ys = []
    for b in range(B):
        n = counts[b]
        m64 = [m[b:b + 1, :, :n].double().cpu() for m in masks] if drop else None
        ys.append(O.transformer_encoder(p64, "e", x64[:, b:b + 1], kv64[:n, b:b + 1], kv64[:n, b:b + 1], T, m64))
    yr = torch.cat(ys, 1)
    (yr * w.double().cpu().reshape(Sq, B, H)).sum().backward()
    rel = lambda a_, b_: float((a_.detach().cpu().double().reshape(b_.shape) - b_.detach()).abs().max() / (b_.detach().abs().max() + 1e-12))
    figs = dict(y=rel(y, yr), dx=rel(dx, x64.grad), dkv=rel(dkv_raw, kv64.grad))
    for b in range(B):                                    # key rows past a crystal's count get no gradient at all
        assert bool((dkv.reshape(Nk, B, H)[counts[b]:, b] == 0).all())
    for k in P:
        figs[k] = rel(G[k], p64[k.replace("enc.", "e.", 1)].grad)
    print(shape, "drop" if drop else "nodrop", off, {k: f"{v:.1e}" for k, v in figs.items()})
    return figs


# test_gpu_ffn.py's bounds for the unflagged encoder (test_attention_fused_into_ffn_matches_two_launches), every figure relative
# to the reference tensor's maximum: 5e-6 on the output, 2e-5 on dx and the key gradient, 5e-5 on the parameter gradients
ENC_Y_TOL, ENC_DX_TOL, ENC_G_TOL = 5e-6, 2e-5, 5e-5


def _enc_assert(figs):
    assert figs.pop("y") < ENC_Y_TOL
    assert figs.pop("dx") < ENC_DX_TOL and figs.pop("dkv") < ENC_DX_TOL
    assert max(figs.values()) < ENC_G_TOL, figs


@pytest.mark.parametrize("drop", [False, True], ids=["nodrop", "drop"])
@pytest.mark.parametrize("shape", ["nk16_h64", "nk37_h128"])
def test_encoder_over_own_keys(shape, drop):
    figs = _encoder_case(shape, drop)
    _enc_assert(figs)


@pytest.mark.parametrize("drop", [False, True], ids=["nodrop", "drop"])
@pytest.mark.parametrize("off", ["_FUSED_ATT_FFN", "_ATT_ALIGNED", "_FUSED_ATT_BWD"])
def test_encoder_over_own_keys_on_separate_launches(off, drop):
    from dostransformer_amd import functional as Fn
    with Fn.forms(**{off: False}):
        _enc_assert(_encoder_case("nk37_h64", drop, off))


# ------------------------------------------------------------------------------------------------------------------
# model level: Trainer(model, per_crystal_keys=True)
# ------------------------------------------------------------------------------------------------------------------
from tests.util import rmse  # noqa: E402

DOS_RMSE = 1e-4                     # the project's north star
F64_MAX, F64_P99, F64_MEDIAN = 3e-3, 1e-3, 1e-4     # test_gpu_models._f64_errors' rule
BATCH1_TOL = 4e-6                   # tests/test_gpu_predict.py:73-75
MODELS = {
    "ph_h16": dict(kind="phonon", n_atoms=[1, 2, 17, 33], L=2, T=1, H=16, seed=31),
    "ph_h64": dict(kind="phonon", n_atoms=[2, 5, 16, 70], L=2, T=2, H=64, seed=32),
    "ed_h64": dict(kind="edos", n_atoms=[1, 15, 16, 36], L=2, T=1, H=64, seed=33),
    "ed_h32": dict(kind="edos", n_atoms=[3, 40, 63, 70], L=2, T=2, H=32, seed=34),      # 71 keys: the streamed kernels
}
BETA = 1.0


def _crystals(name):
    from dostransformer_amd import synth
    c = MODELS[name]
    gen = torch.Generator().manual_seed(c["seed"])
    if c["kind"] == "phonon":
        return [synth.phonon_crystal(gen, n, dtype=torch.float32) for n in c["n_atoms"]]
    return [synth.edos_crystal(gen, n, dtype=torch.float32, idx=i) for i, n in enumerate(c["n_atoms"])]


def _collate(cs):
    from dostransformer_amd.batch import collate
    return collate(cs)


def _model(name, attn_drop=0.0):
    """fp32 module on the GPU and the exact float64 copies of its parameters for the oracle."""
    c = MODELS[name]
    torch.manual_seed(c["seed"])
    if c["kind"] == "phonon":
        from dostransformer_amd.embedder_phDOS.DOSTransformer_phonon import DOSTransformer_phonon
        model = DOSTransformer_phonon(c["L"], c["T"], 118, 4, c["H"], DEV, attn_drop)
    else:
        from dostransformer_amd.embedder_eDOS.DOSTransformer import DOSTransformer
        model = DOSTransformer(c["L"], c["T"], 200, 41, 2, c["H"], DEV, attn_drop)
    p = {k: (v.detach().clone().double() if v.is_floating_point() else v.clone()) for k, v in model.state_dict().items()}
    return model.to(DEV), p


def _leaves(p):
    return {k: v.clone().requires_grad_(True) for k, v in p.items()
            if v.is_floating_point() and k != "version" and not k.endswith(".version")}


def _oracle_fwd(kind, leaves, g64, L, T, masks=None):
    from oracle import dos_oracle as O
    f = O.dostransformer_phonon_forward if kind == "phonon" else O.dostransformer_forward
    return f(leaves, g64, L, T, masks)


def _oracle_loss(kind, dg, ds, g64):
    from oracle import dos_oracle as O
    return O.loss_phonon(dg, ds, g64.phdos, BETA) if kind == "phonon" else O.loss_edos(dg, ds, g64.y_ft, BETA)


def _oracle_batch1(name, p, masks=None):
    """The oracle on every crystal alone; its loss on the concatenated batch-1 outputs; the autograd gradient of that loss through
    the B batch-1 forwards.  masks: the logged [Bq, S, Nk] masks of the batched run - crystal b alone gets rows [b, B + b]
    (transformer: [b]) and columns [:n_b]."""
    c = MODELS[name]
    kind = c["kind"]
    cs = _crystals(name)
    B = len(cs)
    leaves = _leaves(p)
    gall = _collate(cs).to("cpu", dtype=torch.float64)
    dgs, dss = [], []
    for b, cr in enumerate(cs):
        n = c["n_atoms"][b] + (1 if kind == "edos" else 0)        # eDOS: the phantom node counts as an atom
        mb = None
        if masks is not None:
            mb = {"transformer": [m[b:b + 1, :, :n] for m in masks["transformer"]],
                  "transformer_self": [m[[b, B + b]] for m in masks["transformer_self"]],
                  "transformer_source": [m[[b, B + b]][:, :, :n] for m in masks["transformer_source"]]}
        dg, _, ds = _oracle_fwd(kind, leaves, _collate([cr]).to("cpu", dtype=torch.float64), c["L"], c["T"], mb)
        dgs.append(dg)
        dss.append(ds)
    dg, ds = torch.cat(dgs), torch.cat(dss)
    loss = _oracle_loss(kind, dg, ds, gall)
    names = list(leaves)
    gr = torch.autograd.grad(loss, [leaves[k] for k in names], allow_unused=True)
    return dg.detach(), ds.detach(), float(loss.detach()), dict(zip(names, gr))


def _oracle_batched(name, p):
    c = MODELS[name]
    leaves = _leaves(p)
    g64 = _collate(_crystals(name)).to("cpu", dtype=torch.float64)
    dg, _, ds = _oracle_fwd(c["kind"], leaves, g64, c["L"], c["T"])
    loss = _oracle_loss(c["kind"], dg, ds, g64)
    names = list(leaves)
    gr = torch.autograd.grad(loss, [leaves[k] for k in names], allow_unused=True)
    return dg.detach(), ds.detach(), float(loss.detach()), dict(zip(names, gr))


def _grad_errors(label, G, grads64):
    """test_gpu_models._f64_errors' element-error rule on the live gradients: (max, p99, median) of |got - ref| / max|ref|,
    the last two over tensors of >= 256 elements; dead parameters are absent from G."""
    worst, w99, w50 = (0.0, None), (0.0, None), (0.0, None)
    for k, r in grads64.items():
        if r is None:
            assert k not in G, k
            continue
        e = ((G[k].detach().cpu().double() - r).abs() / (r.abs().max() + 1e-6)).reshape(-1)
        worst = max(worst, (float(e.max()), k))
        if e.numel() >= 256:
            w99 = max(w99, (float(torch.quantile(e[:1 << 24], 0.99)), k))
            w50 = max(w50, (float(e.median()), k))
    print(f"{label}: gradients worst {worst[0]:.3e} at {worst[1]}; p99 {w99[0]:.3e} at {w99[1]}; median {w50[0]:.3e} at {w50[1]}")
    return worst, w99, w50


def _assert_grads(label, G, grads64):
    w, w99, w50 = _grad_errors(label, G, grads64)
    assert w[0] < F64_MAX and w99[0] < F64_P99 and w50[0] < F64_MEDIAN, (w, w99, w50)


@pytest.mark.parametrize("name", list(MODELS))
def test_trainer_per_crystal_keys_equals_the_batch_1_oracle(name):
    from dostransformer_amd.train import Trainer
    c = MODELS[name]
    kind = c["kind"]
    cs = _crystals(name)
    B = len(cs)
    model, p = _model(name)
    rg, rs, rloss, rgrads = _oracle_batch1(name, p)
    # ---- input condition (CPU): the flag cannot be ignored ----
    bg, bs, bloss, bgrads = _oracle_batched(name, p)
    nmax = max(c["n_atoms"])
    diffs = [min(rmse(bg[b], rg[b]), rmse(bs[b], rs[b])) for b, n in enumerate(c["n_atoms"]) if n < nmax]
    med = []
    for k, r in rgrads.items():
        if r is not None:
            med.append(float((bgrads[k] - r).abs().max() / (r.abs().max() + 1e-300)))
    med = float(torch.tensor(med).median())
    print(f"{name}: batched vs batch-1 oracle: smallest DOS RMSE of a padded crystal {min(diffs):.2e}, median gradient difference {med:.2f}")
    assert len(diffs) == B - 1 and min(diffs) >= 5e-3, diffs
    assert med >= 0.1, med
    # ---- the flagged trainer against the batch-1 oracle ----
    g = _collate(cs).to(DEV)
    tr = Trainer(model, beta=BETA, per_crystal_keys=True)
    loss = tr.forward_backward(g)
    dg, _, ds = tr.last_outputs
    for b in range(B):
        e = (rmse(dg[b].cpu(), rg[b]), rmse(ds[b].cpu(), rs[b]))
        assert max(e) < DOS_RMSE, (name, b, e)
    print(f"{name}: loss {float(loss):.8f} oracle {rloss:.8f}")
    assert abs(float(loss) - rloss) < (1 + BETA) * 1e-4
    _assert_grads(name, model.flat_params().G, rgrads)
    g1 = model.flat_params().grad.clone()
    # ---- each crystal against the GPU's own unflagged forward on the crystal alone ----
    model.eval()
    with torch.no_grad():
        for b, cr in enumerate(cs):
            og, _, os_ = model(_collate([cr]).to(DEV))
            for got, ref in ((dg[b], og[0]), (ds[b], os_[0])):
                assert float((got - ref).abs().max()) <= BATCH1_TOL * max(float(ref.abs().max()), 1.0), (name, b)
    model.train()
    # ---- two flagged runs are bitwise equal ----
    loss2 = tr.forward_backward(g)
    assert float(loss2) == float(loss) and torch.equal(model.flat_params().grad, g1)
    assert all(torch.equal(a, b_) for a, b_ in zip((dg, ds), (tr.last_outputs[0], tr.last_outputs[2])))
    # ---- the unflagged trainer on the same batch still is the batched oracle ----
    plain, _ = _model(name)
    tp = Trainer(plain, beta=BETA)
    assert tp.per_crystal_keys is False
    lp = tp.forward_backward(g)
    pg, _, ps = tp.last_outputs
    assert rmse(pg.cpu(), bg) < DOS_RMSE and rmse(ps.cpu(), bs) < DOS_RMSE
    assert abs(float(lp) - bloss) < (1 + BETA) * 1e-4
    _assert_grads(name + " unflagged", plain.flat_params().G, bgrads)


def test_trainer_per_crystal_keys_with_attention_dropout(monkeypatch):
    """attn_drop 0.25 in train mode (phonon h16): the masks are drawn on [Bq, S, n_max] as without the flag; the oracle alone on
    crystal b gets rows [b, B + b] and columns [:n_b] of each logged mask.  Same bounds."""
    from dostransformer_amd import functional as Fn
    from dostransformer_amd.train import Trainer
    name = "ph_h16"
    c = MODELS[name]
    cs = _crystals(name)
    B, T, nmax, S = len(cs), c["T"], max(c["n_atoms"]), 51
    model, p = _model(name, attn_drop=0.25)
    model.train()
    monkeypatch.setattr(Fn, "DROP_MASK_LOG", [])
    tr = Trainer(model, beta=BETA, per_crystal_keys=True)
    loss = tr.forward_backward(_collate(cs).to(DEV))
    log = Fn.DROP_MASK_LOG
    assert len(log) == 3 * T
    masks = {pre: [m.detach().cpu().double() for (pr, t, m) in log if pr == pre] for pre in
             ("transformer", "transformer_self", "transformer_source")}
    assert tuple(masks["transformer"][0].shape) == (B, S, nmax)
    assert tuple(masks["transformer_source"][0].shape) == (2 * B, S, nmax)
    assert float(masks["transformer_source"][0].min()) == 0.0            # something was dropped
    rg, rs, rloss, rgrads = _oracle_batch1(name, p, masks)
    dg, _, ds = tr.last_outputs
    for b in range(B):
        assert max(rmse(dg[b].cpu(), rg[b]), rmse(ds[b].cpu(), rs[b])) < DOS_RMSE, b
    assert abs(float(loss) - rloss) < (1 + BETA) * 1e-4
    _assert_grads("dropout", model.flat_params().G, rgrads)


@pytest.mark.parametrize("mode", ["replay", "graph"])
@pytest.mark.parametrize("name", ["ph_h64", "ed_h64"])
def test_flagged_replay_and_graph_steps_equal_the_eager_step(name, mode):
    """A flagged step with replay=True (graph=True) equals the eager flagged step bitwise: loss, flat gradients, parameters after
    step().  The eager step runs on the batch padded to the recorded bucket (the ghost rows are exact)."""
    from dostransformer_amd.batch import bucket_sizes, pad_batch
    from dostransformer_amd.train import Trainer
    cs = _crystals(name)
    gh = _collate(cs)
    res = []
    for m in ("eager", mode):
        model, _ = _model(name)
        tr = Trainer(model, beta=BETA, per_crystal_keys=True, replay=(m == "replay"), graph=(m == "graph"))
        g = gh.to(DEV) if m != "eager" else pad_batch(gh, *bucket_sizes(gh.meta.num_nodes, gh.meta.num_edges, *tr.bucket)).to(DEV)
        loss = tr.step(g)
        loss = tr.step(g)                     # (the second step replays the recording)
        torch.cuda.synchronize()
        res.append((float(loss), model.flat_params().grad.clone(), model.flat_params().flat.clone()))
    assert res[0][0] == res[1][0]
    assert torch.equal(res[0][1], res[1][1]) and torch.equal(res[0][2], res[1][2])


def test_flagged_ghost_padded_bucket_equals_eager():
    """replay=True, bucket (8, 128): the batch is ghost-padded to its bucket and the bucket's own graph_ptr is the operand.  Loss,
    flat gradients and the parameters after step() equal the eager flagged step on the batch padded to that bucket bitwise;
    against the eager step on the unpadded batch the loss and every crystal's DOS are bitwise too (its weight-gradient slabs
    split at other rows, so its gradient sums are ordered differently - as without the flag, test_gpu_models)."""
    from dostransformer_amd.batch import bucket_sizes, pad_batch
    from dostransformer_amd.train import Trainer
    name = "ph_h64"
    gh = _collate(_crystals(name))
    gp = pad_batch(gh, *bucket_sizes(gh.meta.num_nodes, gh.meta.num_edges, 8, 128)).to(DEV)
    assert gp.meta.num_nodes > gh.meta.num_nodes                               # there are ghost rows
    res = []
    for mode in ("eager", "replay"):
        model, _ = _model(name)
        tr = Trainer(model, beta=BETA, per_crystal_keys=True, replay=(mode == "replay"), bucket=(8, 128))
        loss = tr.step(gp if mode == "eager" else gh.to(DEV))
        torch.cuda.synchronize()
        res.append((float(loss), model.flat_params().grad.clone(), model.flat_params().flat.clone(),
                    tr.last_outputs[0].clone(), tr.last_outputs[2].clone()))
    assert res[0][0] == res[1][0]
    for u, v in zip(res[0][1:], res[1][1:]):
        assert torch.equal(u, v)
    model, _ = _model(name)
    te = Trainer(model, beta=BETA, per_crystal_keys=True)
    le = te.forward_backward(gh.to(DEV))
    assert float(le) == res[1][0]
    assert torch.equal(te.last_outputs[0], res[1][3]) and torch.equal(te.last_outputs[2], res[1][4])


@pytest.mark.parametrize("name", ["ph_h64", "ed_h32"])
def test_reordering_the_batch_permutes_the_outputs(name):
    from dostransformer_amd.train import Trainer
    cs = _crystals(name)
    perm = [2, 0, 3, 1]
    model, _ = _model(name)
    tr = Trainer(model, beta=BETA, per_crystal_keys=True)
    tr.forward_backward(_collate(cs).to(DEV))
    a = [tr.last_outputs[0].clone(), tr.last_outputs[2].clone()]
    tr.forward_backward(_collate([cs[i] for i in perm]).to(DEV))
    b = [tr.last_outputs[0], tr.last_outputs[2]]
    for u, v in zip(a, b):
        for k, i in enumerate(perm):
            assert float((v[k] - u[i]).abs().max()) <= BATCH1_TOL * max(float(u[i].abs().max()), 1.0), (name, k)


@pytest.mark.parametrize("mode", ["replay", "graph"])
def test_a_recorded_slot_follows_the_next_batch_counts(mode):
    """Two batches of one bucket with DIFFERENT atoms per crystal (same total): the second replays the launch list the first
    recorded.  The recorded key_ptr is the slot's own graph_ptr buffer, so the second batch's loss, gradients and DOS equal its own
    eager flagged step on the padded batch bitwise - a recording that kept the first batch's counts would give the first's."""
    from dostransformer_amd import synth
    from dostransformer_amd.batch import bucket_sizes, pad_batch
    from dostransformer_amd.train import Trainer
    c = MODELS["ph_h64"]
    batches = []
    for seed, n_atoms in ((41, [3, 9, 12, 4]), (42, [12, 2, 5, 9])):                 # 28 atoms, 560 edges each; n_max 12
        gen = torch.Generator().manual_seed(seed)
        batches.append(_collate([synth.phonon_crystal(gen, n, dtype=torch.float32) for n in n_atoms]))
    model, _ = _model("ph_h64")
    tr = Trainer(model, lr=0.0, weight_decay=0.0, beta=BETA, per_crystal_keys=True, replay=(mode == "replay"), graph=(mode == "graph"))
    got = []
    for g in batches:
        loss = tr.step(g.to(DEV))
        torch.cuda.synchronize()
        got.append((float(loss), model.flat_params().grad.clone(), tr.last_outputs[0].clone(), tr.last_outputs[2].clone()))
    assert len(tr._slots) == 1                                                        # the second batch replayed the first's recording
    assert got[0][0] != got[1][0]
    me, _ = _model("ph_h64")
    te = Trainer(me, lr=0.0, weight_decay=0.0, beta=BETA, per_crystal_keys=True)
    for g, want in zip(batches, got):
        gp = pad_batch(g, *bucket_sizes(g.meta.num_nodes, g.meta.num_edges, *tr.bucket)).to(DEV)
        loss = te.step(gp)
        torch.cuda.synchronize()
        assert float(loss) == want[0]
        assert torch.equal(me.flat_params().grad, want[1])
        assert torch.equal(te.last_outputs[0], want[2]) and torch.equal(te.last_outputs[2], want[3])


def test_hidden_above_the_attention_row_width_is_refused_under_the_flag():
    from dostransformer_amd import ops as O_
    from dostransformer_amd import synth
    from dostransformer_amd._lib import DosxError
    from dostransformer_amd.embedder_phDOS.DOSTransformer_phonon import DOSTransformer_phonon
    from dostransformer_amd.train import Trainer
    H = O_.ATTN_MAX_H + 64
    model = DOSTransformer_phonon(1, 1, 118, 4, H, DEV, 0.0).to(DEV)
    g = synth.phonon_batch(2, seed=5, dtype=torch.float32, n_atoms=[2, 3]).to(DEV)
    with pytest.raises(DosxError, match="per_crystal_keys"):
        Trainer(model, per_crystal_keys=True).forward_backward(g)
    assert torch.isfinite(Trainer(model).forward_backward(g))                         # (without the flag the wide path runs)
