"""The three launches whose dynamic-LDS request used to be remembered per PROCESS, on a second device of a process that
has already run them on the first (csrc/launch_state.h keeps the grant per device): k_fbank_center_span at its largest
window (146 KB), k_lstm_rec_gen at H = 256 (66.5 KB) and k_stats_pool_rows_long (up to 144 KB).  Needs two GPUs."""
import pytest
import torch

from kernel_parity import SEED_OFFSET
from lstm_cases import run_kernel, saturating_case

pytestmark = pytest.mark.gpu


def _three_launches(device):
    import xvector_mfcc_oracle as xo
    import pyannote_audio_amd as pa
    import pyannote_audio_amd.ffi as ffi
    lib = ffi.load()
    g = torch.Generator().manual_seed(8100 + SEED_OFFSET)
    out = {}
    with torch.cuda.device(device):
        # B = 1, T = 1100, 80 mel bins, a running mean over 2049 frames
        x = (4.0 * torch.randn(1, 1100, 80, generator=g) - 9.0).to(device)
        centred = torch.full_like(x, float("nan"))
        ffi.check(lib.pa_fbank_center_span(ffi.ptr(x), 1, 1100, 80, 2049, ffi.ptr(centred), ffi.stream()),
                  f"center_span on {device}")
        torch.cuda.synchronize()
        out["fbank_center_span"] = centred.cpu()
        pre, whh = saturating_case(256, 1, 4, 1.0, 0.0, 1.0, 16, 0)
        out["lstm_rec_h"] = run_kernel(pre, whh, device, f"lstm H256 on {device}")
    # the long pooling kernel has no entry point of its own: the x-vector forward on the shortest chunk that has more
    # pool frames than k_stats_pool_rows takes (640)
    oracle = xo.seeded_xvector_mfcc(seed=3579)
    model = pa.XVectorMFCC(oracle.state_dict(), xo.xvector_mfcc_hparams(oracle), pa.model.embedding_specifications())
    N = next(n for n in range(100000, 160001, 100) if model.num_frames(n) == 641)
    wav = (0.1 * torch.randn(1, 1, N, generator=g)).clamp(-1, 1)
    w = torch.rand(1, 2, 641, generator=g)
    out["xvec_long_pool"] = model.to(device)(wav.to(device), w.to(device)).cpu()
    for name, value in out.items():
        assert torch.isfinite(value).all(), f"{name} on {device}"
    return out


def test_second_device_repeats_the_first(gpu_device):
    if torch.cuda.device_count() < 2:
        pytest.skip("needs two GPUs: the per-device LDS grant shows only on a second device of one process")
    first = _three_launches(torch.device("cuda:0"))
    second = _three_launches(torch.device("cuda:1"))
    for name in first:
        assert torch.equal(second[name], first[name]), name
