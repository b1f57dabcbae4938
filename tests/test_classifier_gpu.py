"""k_classifier (csrc/seg_lstm.hip) through pa_classifier, on its own: Linear(K -> NC) + log-softmax + powerset look-up,
or + sigmoid for multi-label heads, on a (tile, t, b16)-ordered activation matrix.  Truth: float64 logits,
log_softmax / sigmoid and argmax.  Rules of the comparison: tests/kernel_parity.py."""
import pytest
import torch

from kernel_parity import SEED_OFFSET, Guarded, assert_parity, dptr, ratio

pytestmark = pytest.mark.gpu

NCS, KS, TS, BS = (1, 2, 7, 11, 16), (4, 32, 128, 512), (1, 37, 589), (1, 16, 17, 37)


def _ri(rng, lo, hi):
    return int(torch.randint(lo, hi + 1, (1,), generator=rng))


def _cases():
    """28 seeded draws from NC x K x ldx x T x B x S x {both outputs, logp NULL, multilabel NULL}; the first 20 walk
    through every value of every list, whatever the seed"""
    rng = torch.Generator().manual_seed(8100 + SEED_OFFSET)
    cases = []
    for i in range(28):
        pick = (lambda lst, j: lst[j % len(lst)]) if i < 20 else (lambda lst, j: lst[_ri(rng, 0, len(lst) - 1)])
        K = pick(KS, i)
        cases.append(dict(NC=pick(NCS, i), K=K, ldx=K + 4 * (i // 4 % 2), T=pick(TS, i // 2), B=pick(BS, i // 3),
                          S=1 + (i // 5) % 4, outputs=("both", "logp", "ml")[i % 3], exact=i % 2 == 0,
                          seed=8200 + i + SEED_OFFSET))
    return cases


def test_case_list_covers_every_value():
    cases = _cases()
    for key, values in (("NC", NCS), ("K", KS), ("T", TS), ("B", BS), ("S", (1, 2, 3, 4))):
        assert {c[key] for c in cases} == set(values), key
    assert {c["ldx"] - c["K"] for c in cases} == {0, 4}
    assert {c["outputs"] for c in cases} == {"both", "logp", "ml"}
    assert {(c["exact"], c["outputs"]) for c in cases} >= {(e, o) for e in (True, False) for o in ("both", "logp", "ml")}


def _operands(NC, K, ldx, T, B, exact, seed, reach):
    """X in (tile, t, b16) row order with NaN padding columns, classifier weights and bias.
    exact: inputs on a dyadic grid, so that every float32 product and partial sum of the logits is exact and logits of
    +-`reach` say nothing about summation order -- what is measured is the softmax.  Otherwise Gaussian operands with
    logits of a few units, where float32 summation is within the contract."""
    rng = torch.Generator().manual_seed(seed)
    ntiles = (B + 15) // 16
    rows = ntiles * T * 16
    X = torch.full((rows, ldx), float("nan"))
    if exact:
        X[:, :K] = torch.randint(-4, 5, (rows, K), generator=rng).float() / 4
        # logit = sum of K terms of standard deviation ~0.65 x 0.61 s: s = the power of two that brings 3.3 sigma to `reach`
        s = 2.0 ** round(torch.log2(torch.tensor(reach / 3.3 / (0.4 * K ** 0.5))).item())
        cw = torch.randint(-8, 9, (NC, K), generator=rng).float() / 8 * s
        cb = torch.randint(-8, 9, (NC,), generator=rng).float() / 8 * s
    else:
        X[:, :K] = torch.randn(rows, K, generator=rng)
        cw = torch.randn(NC, K, generator=rng) * (2.0 / K ** 0.5)
        cb = torch.randn(NC, generator=rng)
    return X, cw, cb


def _logits(X, cw, cb, K, T, B, dtype):
    """(B, T, NC) logits of the real chunks"""
    ntiles = X.shape[0] // (16 * T)
    z = X[:, :K].to(dtype) @ cw.to(dtype).T + cb.to(dtype)
    return z.view(ntiles, T, 16, -1).permute(0, 2, 1, 3).reshape(ntiles * 16, T, -1)[:B]


def _run(lib, ffi, dev, X, cw, cb, c, mapping, want_logp, want_ml):
    NC, K, T, B, S = c["NC"], c["K"], c["T"], c["B"], c["S"]
    ntiles = (B + 15) // 16
    Xd, cwd, cbd = X.to(dev), cw.to(dev), cb.to(dev)
    md = mapping.to(dev) if mapping is not None else None
    logp = Guarded(B * T * NC, dev)
    ml = Guarded(B * T * S, dev, torch.uint8)
    rc = lib.pa_classifier(dptr(Xd), c["ldx"], K, ntiles, T, B, dptr(cwd), dptr(cbd), NC, dptr(md), S,
                           logp.ptr if want_logp else None, ml.ptr if want_ml else None, ffi.stream())
    ffi.check(rc, f"pa_classifier {c}")
    # rows of the chunks that pad the last tile (b >= B) would land behind the outputs: the guards catch them
    got_logp = logp.check(None, f"logp {c}").view(B, T, NC) if want_logp else None
    got_ml = ml.check(None, f"multilabel {c}").view(B, T, S) if want_ml else None
    if not want_logp:
        assert logp.untouched()
    if not want_ml:
        assert ml.untouched()
    return got_logp, got_ml


@pytest.mark.parametrize("block", range(4))
def test_classifier_powerset(gpu_device, block):
    """log-probabilities finite and within the contract of float64 log_softmax for logits up to +-80; hard decision =
    the mapping row of the float64 argmax wherever the top-2 gap exceeds 1e-4"""
    import pyannote_audio_amd.ffi as ffi
    lib = ffi.load()
    reached = 0.0
    for c in _cases()[block * 7:(block + 1) * 7]:
        X, cw, cb = _operands(c["NC"], c["K"], c["ldx"], c["T"], c["B"], c["exact"], c["seed"], reach=80.0)
        mapping = torch.randint(0, 2, (c["NC"], c["S"]), generator=torch.Generator().manual_seed(c["seed"]),
                                dtype=torch.uint8)
        z64 = _logits(X, cw, cb, c["K"], c["T"], c["B"], torch.float64)
        z32 = _logits(X, cw, cb, c["K"], c["T"], c["B"], torch.float32)
        truth, ref32 = torch.log_softmax(z64, -1), torch.log_softmax(z32, -1)
        if c["exact"]:
            assert torch.equal(z32.double(), z64)       # the dyadic grid does what it is there for
            reached = max(reached, z64.abs().max().item())
        got_logp, got_ml = _run(lib, ffi, gpu_device, X, cw, cb, c, mapping, c["outputs"] != "ml", c["outputs"] != "logp")
        tag = "classifier_NC{NC}_K{K}_ldx{ldx}_T{T}_B{B}_S{S}_{outputs}".format(**c) + ("_exact" if c["exact"] else "")
        if got_logp is not None:
            assert torch.isfinite(got_logp).all(), c
            assert_parity(tag, got_logp, truth, ref32)
        else:
            assert ratio(ref32, truth) <= 0.5, c
        if got_ml is not None:
            if c["NC"] > 1:
                top2 = z64.topk(2, dim=-1).values
                safe = (top2[..., 0] - top2[..., 1]) > 1e-4
            else:
                safe = torch.ones(z64.shape[:2], dtype=torch.bool)
            want = mapping[z64.argmax(-1)]
            assert safe.numel() < 100 or safe.float().mean() > 0.9, c
            assert torch.equal(got_ml[safe], want[safe]), c
    # (each block of seven holds an exact case whose logits reach the +-80 the test is about)
    assert reached >= 60.0, reached


def test_classifier_exact_ties_go_to_the_lower_class(gpu_device):
    """two classes with identical weight rows and bias: where they share the maximum the lower index wins, as
    torch.argmax does on the CPU -- whichever two positions the twins sit at, the first and the last class included"""
    import pyannote_audio_amd.ffi as ffi
    lib = ffi.load()
    for i, (NC, lo, hi) in enumerate(((2, 0, 1), (7, 0, 6), (7, 2, 5), (16, 0, 15), (16, 14, 15), (11, 3, 4))):
        c = dict(NC=NC, K=32, ldx=36, T=37, B=17, S=3, seed=8300 + i + SEED_OFFSET)
        X, cw, cb = _operands(NC, 32, 36, 37, 17, True, c["seed"], reach=20.0)
        cw[hi], cb[hi] = cw[lo], cb[lo]
        others = [k for k in range(NC) if k not in (lo, hi)]
        cw[others] = cw[others] / 4          # the twins win about half of the rows
        cb[others] = cb[others] / 4
        mapping = torch.zeros(NC, 3, dtype=torch.uint8)
        mapping[:, 0] = torch.arange(NC) % 2
        mapping[lo], mapping[hi] = torch.tensor([1, 0, 1], dtype=torch.uint8), torch.tensor([0, 1, 1], dtype=torch.uint8)
        z64 = _logits(X, cw, cb, 32, 37, 17, torch.float64)
        rest = z64[..., others].max(-1).values if others else torch.full(z64.shape[:2], -float("inf"), dtype=z64.dtype)
        tied = z64[..., lo] > rest                      # the twins, and only they, hold the maximum
        assert torch.equal(z64[..., lo], z64[..., hi]) and tied.float().mean() > 0.2
        assert bool((z64.argmax(-1)[tied] == lo).all())                 # torch's own convention on the CPU
        got_logp, got_ml = _run(lib, ffi, gpu_device, X, cw, cb, c, mapping, True, True)
        assert torch.equal(got_ml[tied], mapping[lo].expand(int(tied.sum()), 3)), (NC, lo, hi)
        assert_parity(f"classifier_ties_NC{NC}_{lo}_{hi}", got_logp, torch.log_softmax(z64, -1),
                      torch.log_softmax(_logits(X, cw, cb, 32, 37, 17, torch.float32), -1))


@pytest.mark.parametrize("NC,K,T,B", [(1, 4, 589, 17), (3, 32, 37, 37), (7, 128, 589, 16), (16, 512, 37, 1)])
def test_classifier_multilabel_sigmoid(gpu_device, NC, K, T, B):
    """mapping == NULL: sigmoid scores against float64 for logits up to +-100; no NaN; exactly 1 only where the float64
    value has 1.0f as a float32 neighbour (> 1 - 2^-24: 1 / (1 + e) in float32 is faithfully, not correctly, rounded),
    exactly 0 only below the smallest normal float32 (1.18e-38: GPUs may flush what lies below it); the multilabel
    output is not written"""
    import pyannote_audio_amd.ffi as ffi
    lib = ffi.load()
    c = dict(NC=NC, K=K, ldx=K + 4, T=T, B=B, S=NC, seed=8400 + NC + SEED_OFFSET)
    X, cw, cb = _operands(NC, K, K + 4, T, B, True, c["seed"], reach=100.0)
    z64 = _logits(X, cw, cb, K, T, B, torch.float64)
    assert torch.equal(_logits(X, cw, cb, K, T, B, torch.float32).double(), z64) and z64.abs().max() >= 60.0
    truth = torch.sigmoid(z64)
    got, _ = _run(lib, ffi, gpu_device, X, cw, cb, c, None, True, False)
    assert_parity(f"classifier_sigmoid_NC{NC}_K{K}_T{T}_B{B}", got, truth, torch.sigmoid(z64.float()))
    assert bool((truth[got == 1.0] > 1.0 - 2.0 ** -24).all())
    assert bool((truth[got == 0.0] < 2.0 ** -126).all())
    assert bool((got >= 0).all()) and bool((got <= 1).all())


def test_classifier_weights_beyond_64_kb_of_lds(gpu_device):
    """16 classes (5 speakers, at most 2 at a time) on a 512-wide bidirectional LSTM without a Linear head: K = 1024,
    (16 x 1024 + 16) x 4 = 65 600 bytes of dynamic LDS, 64 more than the 64 KB the launcher never asks to exceed.
    SegmentationPack accepts that checkpoint, so the call has to work -- and it does: the runtime grants a launch its
    dynamic LDS up to the device's 160 KB without a hipFuncSetAttribute.  The test pins that."""
    import pyannote_audio_amd.ffi as ffi
    lib = ffi.load()
    c = dict(NC=16, K=1024, ldx=1024, T=37, B=17, S=5, seed=8500 + SEED_OFFSET)
    X, cw, cb = _operands(16, 1024, 1024, 37, 17, False, c["seed"], reach=0.0)
    mapping = torch.randint(0, 2, (16, 5), generator=torch.Generator().manual_seed(c["seed"]), dtype=torch.uint8)
    z64 = _logits(X, cw, cb, 1024, 37, 17, torch.float64)
    got_logp, got_ml = _run(lib, ffi, gpu_device, X, cw, cb, c, mapping, True, True)
    assert_parity("classifier_NC16_K1024", got_logp, torch.log_softmax(z64, -1),
                  torch.log_softmax(_logits(X, cw, cb, 1024, 37, 17, torch.float32), -1))
    top2 = z64.topk(2, dim=-1).values
    safe = (top2[..., 0] - top2[..., 1]) > 1e-4
    assert torch.equal(got_ml[safe], mapping[z64.argmax(-1)][safe])
    # ... and the smaller request of every other checkpoint still works afterwards
    c = dict(NC=7, K=128, ldx=128, T=37, B=17, S=3, seed=8501 + SEED_OFFSET)
    X, cw, cb = _operands(7, 128, 128, 37, 17, False, c["seed"], reach=0.0)
    got_logp, _ = _run(lib, ffi, gpu_device, X, cw, cb, c, mapping[:7, :3].contiguous(), True, True)
    assert_parity("classifier_NC7_K128_after_NC16_K1024", got_logp,
                  torch.log_softmax(_logits(X, cw, cb, 128, 37, 17, torch.float64), -1),
                  torch.log_softmax(_logits(X, cw, cb, 128, 37, 17, torch.float32), -1))
