"""Child process of tests/test_stream_contract_gpu.py::test_first_persistent_convolution_of_a_process_on_a_side_stream
(TEST INFRASTRUCTURE ONLY; run as a script, never imported).

Its first call into libpyannote_amd.so is pa_conv3x3 on a non-blocking side stream: the first-use path of the
tile-counter pool.  The case is the exact integer one of tests/conv_truth.py in which every claiming workgroup takes at
least two tiles; the output must equal the integer convolution bit for bit.  Prints COLD START OK and exits 0, or says
what differed and exits 1."""
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path[:0] = [os.path.dirname(HERE), HERE]

import torch  # noqa: E402

import conv_truth as T  # noqa: E402
from kernel_parity import Guarded, dptr  # noqa: E402


def main() -> int:
    import pyannote_audio_amd.ffi as ffi
    ffi.require_gpu()
    lib = ffi.load()                                      # dlopen only: no entry point has been called yet
    dev = torch.device("cuda:0")
    case = next(c for c in T.CASES if c["name"] == "direct_16to32_3x5_B1024")
    assert case["many"] and T.workgroup_tiles(case) >= 2 * T.CLAIMERS["direct"]
    x, w, shift, R = T.exact_inputs(case, T.exact_seed(case, 0), 0)
    _, packed = T.exact_image(case, w)
    use_res, relu = case["variants"][0]
    truth = T.exact_truth(case, x, w, shift, R, use_res, relu)
    nhwc = lambda t: t.permute(0, 2, 3, 1).contiguous().to(dev)
    xd, wd, shd, rd = nhwc(x), packed.contiguous().to(dev), shift.to(dev), nhwc(R)
    Ho, Wo = T.out_hw(case["H"], case["W"], case["stride"])
    out = Guarded(case["B"] * Ho * Wo * case["cout"], dev)
    torch.cuda.synchronize()                              # the uploads ran on torch's default stream
    side = torch.cuda.Stream()                            # (torch creates its streams non-blocking)
    with torch.cuda.stream(side):
        assert ffi.stream().value == side.cuda_stream
        rc = lib.pa_conv3x3(dptr(xd), case["B"], case["H"], case["W"], case["cin"], dptr(wd), dptr(shd),
                            dptr(rd) if use_res else None, out.ptr, case["cout"], case["stride"], int(relu), ffi.stream())
    if rc != 0:
        print(f"pa_conv3x3 returned {rc}: {lib.pa_last_error().decode()}")
        return 1
    side.synchronize()
    got = out.check(None, "cold start").view(case["B"], Ho, Wo, case["cout"]).permute(0, 3, 1, 2)
    if not torch.equal(got, truth):
        bad = got != truth
        print(f"{int(bad.sum())} of {bad.numel()} outputs differ from the integer convolution, first at "
              f"{bad.nonzero()[0].tolist()}")
        return 1
    print("COLD START OK")
    return 0


if __name__ == "__main__":
    sys.exit(main())
