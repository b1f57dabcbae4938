"""What the tests of pa_lstm_rec_h share (tests/test_lstm_values_gpu.py, tests/test_second_device_gpu.py): the float64 /
float32 step loop that is their truth, the call of the kernel on operands laid out as weights.py lays them out, and
the seeded nn.LSTM whose gates saturate."""
import torch

from kernel_parity import SEED_OFFSET, Guarded, dptr


def recurrence(pre, whh, dtype):
    """pre (B, T, ndir, 4H) gate pre-activations in torch's order i, f, g, o; whh: ndir matrices (4H, H); direction 1
    runs backwards in time.  Returns h (B, T, ndir * H), computed step by step in `dtype`."""
    B, T, ndir, H4 = pre.shape
    H = H4 // 4
    out = torch.zeros(B, T, ndir * H, dtype=dtype)
    for d in range(ndir):
        w = whh[d].to(dtype).T.contiguous()
        x = pre[:, :, d].to(dtype)
        h = torch.zeros(B, H, dtype=dtype)
        c = torch.zeros(B, H, dtype=dtype)
        for t in (range(T - 1, -1, -1) if d else range(T)):
            z = x[:, t] + h @ w
            i, f = torch.sigmoid(z[:, :H]), torch.sigmoid(z[:, H:2 * H])
            g, o = torch.tanh(z[:, 2 * H:3 * H]), torch.sigmoid(z[:, 3 * H:])
            c = f * c + i * g
            h = o * torch.tanh(c)
            out[:, t, d * H:(d + 1) * H] = h
    return out


def run_kernel(pre, whh, device, tag):
    """pa_lstm_rec_h on `pre` (B, T, ndir, 4H) / `whh`: operand images of weights.py, output inside guards"""
    import pyannote_audio_amd.ffi as ffi
    from pyannote_audio_amd.weights import (_lstm_row_perm, _lstm_row_perm_gen, _lstm_whh_image, _lstm_whh_image_gen)
    lib = ffi.load()
    B, T, ndir, H4 = pre.shape
    H = H4 // 4
    fast = H == 128 and ndir == 2
    perm = _lstm_row_perm() if fast else _lstm_row_perm_gen(H)
    image = _lstm_whh_image if fast else _lstm_whh_image_gen
    ntiles = (B + 15) // 16
    padded = torch.zeros(ntiles * 16, T, ndir, H4)
    padded[:B] = pre[..., perm]
    # [tile][t][ndir * 4H][16]
    xproj = padded.view(ntiles, 16, T, ndir * H4).permute(0, 2, 3, 1).contiguous().to(device)
    wd = torch.cat([image(w.float().contiguous()) for w in whh]).to(device)
    out = Guarded(ntiles * T * 16 * ndir * H, device)
    ffi.check(lib.pa_lstm_rec_h(dptr(xproj), dptr(wd), out.ptr, ntiles, ndir, T, H, ffi.stream()), tag)
    got = out.check(None, tag)       # (the chunks that pad the last tile are computed and stored like the others)
    return got.view(ntiles, T, 16, ndir * H).permute(0, 2, 1, 3).reshape(ntiles * 16, T, ndir * H)[:B]


def saturating_case(H, ndir, T, scale, fb, xs, B, seed):
    torch.manual_seed(700 + seed + SEED_OFFSET)
    lstm = torch.nn.LSTM(64, H, 1, bidirectional=ndir == 2, batch_first=True).double()
    x = xs * torch.randn(B, T, 64, dtype=torch.float64)
    sd = lstm.state_dict()
    pre, whh = [], []
    for d in range(ndir):
        sfx = "_reverse" if d else ""
        bias = scale * (sd["bias_ih_l0" + sfx] + sd["bias_hh_l0" + sfx])
        bias[H:2 * H] += fb
        pre.append(x @ (scale * sd["weight_ih_l0" + sfx]).T + bias)
        whh.append((scale * sd["weight_hh_l0" + sfx]).float())          # the kernel's operands are float32 ...
    pre = torch.stack(pre, 2).float()                                    # ... and so are its gate inputs
    return pre, whh
