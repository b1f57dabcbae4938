"""Value domain of the LSTM recurrence kernels (csrc/seg_lstm.hip: k_lstm_rec for H = 128 bidirectional, k_lstm_rec_gen
for everything else) through pa_lstm_rec_h.  The test builds the gate pre-activations itself, so the kernel under test
is the recurrence alone: its sigmoid / tanh (v_exp_f32 + v_rcp_f32, argument of tanh clamped at +-15), the cell update
and h W_hh^T.  Truth: an explicit float64 step loop over the same float32 pre-activations and weights.
Rules of the comparison: tests/kernel_parity.py."""
import pytest
import torch

from kernel_parity import SEED_OFFSET, assert_parity
from lstm_cases import recurrence, run_kernel, saturating_case

pytestmark = pytest.mark.gpu


def _gate_grid():
    """pre-activation values: 0, +-1e-6 .. +-1e-1, +-1 .. +-20 in steps of 0.25 (crossing the +-15 clamp of tanh and, for
    tanh(2x), its half), the float32 exp range (+-44, +-88, +-89, +-100) and far beyond it (+-1e4, +-1e30)"""
    pos = [10.0 ** e for e in range(-6, 0)] + [0.25 * k for k in range(1, 81)] + \
          [14.999, 15.001, 7.4995, 7.5005, 44.0, 88.0, 89.0, 100.0, 1e4, 1e30]
    return torch.tensor([0.0] + pos + [-v for v in pos])


@pytest.mark.parametrize("H,ndir", [(128, 2), (64, 2), (32, 1)])
@pytest.mark.parametrize("T", [1, 2])
def test_gate_functions_alone(gpu_device, H, ndir, T):
    """W_hh = 0: h_1 = sig(o) tanh(sig(i) tanh(g)) in closed form (T = 2 adds sig(f) c_1).  One gate position is swept
    over the whole grid while the other three sit at every combination of -4, 0, 4; no NaN / inf, float64 bound."""
    grid = _gate_grid()
    rest = torch.tensor([-4.0, 0.0, 4.0])
    units = []                                                     # (n, 4) pre-activations i, f, g, o of one unit
    for q in range(4):
        a, b, c = torch.meshgrid(rest, rest, rest, indexing="ij")
        others = torch.stack([a.reshape(-1), b.reshape(-1), c.reshape(-1)], 1)          # (27, 3)
        u = torch.empty(grid.numel(), 27, 4)
        u[:, :, [k for k in range(4) if k != q]] = others
        u[:, :, q] = grid.view(-1, 1)
        units.append(u.view(-1, 4))
    units = torch.cat(units)
    n = units.shape[0]
    B = (n + H - 1) // H
    rng = torch.Generator().manual_seed(61 + SEED_OFFSET)
    pre = torch.empty(B, T, ndir, 4, H)
    for t in range(T):
        for d in range(ndir):
            # every (step, direction) sees the whole list, each time in another order and filled up from its start
            order = torch.randperm(n, generator=rng)
            order = torch.cat([order, order[:B * H - n]])
            pre[:, t, d] = units[order].view(B, H, 4).permute(0, 2, 1)
    pre = pre.view(B, T, ndir, 4 * H)
    whh = [torch.zeros(4 * H, H) for _ in range(ndir)]
    truth = recurrence(pre, whh, torch.float64)
    ref32 = recurrence(pre, whh, torch.float32)
    assert torch.isfinite(truth).all()
    got = run_kernel(pre, whh, gpu_device, f"gates H{H} T{T}")
    assert torch.isfinite(got).all()
    assert_parity(f"lstm_gates_alone_H{H}_d{ndir}_T{T}", got, truth, ref32)


#: (H, ndir, T, scale, forget-bias shift, input scale, chunks, seed): the regimes of a seeded nn.LSTM(64, H) that
#: float32 torch itself holds to half the contract (checked on the CPU: e.g. H = 128 (4, 3, 1) is chaotic, float32 is
#: 115 x the contract away from float64 there, and is left out for that reason).  Chunk counts: 1, 2 and 3 tiles of 16,
#: not multiples of 16 (an odd tile count leaves the generic kernel's last workgroup with a single tile).
SATURATING = [
    (128, 2, 589, 1.0, 0.0, 1.0, 16, 0),
    (128, 2, 589, 4.0, 0.0, 1.0, 29, 0),
    (128, 2, 589, 8.0, 3.0, 2.0, 37, 0),
    (64, 2, 300, 1.0, 0.0, 1.0, 20, 0),
    (64, 2, 300, 4.0, 3.0, 1.0, 13, 0),
    (64, 2, 300, 8.0, 3.0, 2.0, 48, 0),
    (32, 1, 589, 1.0, 0.0, 1.0, 16, 0),
    (32, 1, 589, 4.0, 0.0, 1.0, 23, 0),
    (32, 1, 589, 8.0, 3.0, 2.0, 41, 0),
]


@pytest.mark.parametrize("H,ndir,T,scale,fb,xs,B,seed", SATURATING)
def test_saturating_layers(gpu_device, H, ndir, T, scale, fb, xs, B, seed):
    """a whole chunk (589 / 300 steps) of a layer whose gates saturate: weights x scale, forget bias + fb, input x xs"""
    pre, whh = saturating_case(H, ndir, T, scale, fb, xs, B, seed)
    truth = recurrence(pre, whh, torch.float64)
    ref32 = recurrence(pre, whh, torch.float32)
    tag = f"lstm_saturating_H{H}_d{ndir}_T{T}_scale{scale:g}_fb{fb:g}_xs{xs:g}_B{B}"
    beyond6 = (pre.abs() > 6).float().mean().item()
    print(f"{tag}: max |pre-activation of the input| = {pre.abs().max().item():.1f}, {100 * beyond6:.0f} % beyond 6")
    got = run_kernel(pre, whh, gpu_device, tag)
    assert_parity(tag, got, truth, ref32)


def test_lds_grant_follows_the_hidden_size(gpu_device):
    """k_lstm_rec_gen asks for dynamic LDS by hidden size (66.5 KB at H = 256, 132 KB at H = 512) and the grant is
    remembered per device as the largest one given (csrc/launch_state.h): H = 256, 512, 256 in one process, one tile of
    16 chunks, 4 steps, one direction.  A grant that shrank or was skipped shows as a failed launch or as other values:
    every result is held to the float64 recurrence, and the third is the first bit for bit."""
    got = {}
    for call, H in enumerate((256, 512, 256)):
        pre, whh = saturating_case(H, 1, 4, 1.0, 0.0, 1.0, 16, 0)
        truth = recurrence(pre, whh, torch.float64)
        ref32 = recurrence(pre, whh, torch.float32)
        tag = f"lstm_lds_grant_call{call}_H{H}"
        got[call] = run_kernel(pre, whh, gpu_device, tag)
        assert_parity(tag, got[call], truth, ref32)
    assert torch.equal(got[2], got[0])
