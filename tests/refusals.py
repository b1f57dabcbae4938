"""Shared by the GPU tests of the forward entry points: a call that an entry point must refuse gets real, full-size
device buffers -- were it wrongly accepted it would compute in bounds -- and outputs with guard bands; the test then
wants return code 3, the recorded `pa_last_error()` text and outputs (guard bands included) nobody wrote to."""
import math

import torch

GUARD = 256            # elements in front of and behind every output
PATTERN = {torch.float32: 1234.5, torch.uint8: 0xA5, torch.int32: -0x5A5A5A5A}


def altered(struct, **fields):
    """a copy of a ctypes weight struct (the same device pointers) with some integer fields changed"""
    copy = type(struct).from_buffer_copy(struct)
    for name, value in fields.items():
        setattr(copy, name, value)
    return copy


def smallest_accepted(frames, hi=16000):
    """the first sample count for which `frames(n)` is positive"""
    from pyannote_audio_amd.speaker_verification import first_true
    return first_true(lambda n: frames(n) > 0, 1, hi)


def check_refusal(launch, outputs, message, device):
    """`launch(*pointers)` -> return code, one pointer per (shape, dtype) of `outputs`"""
    import pyannote_audio_amd.ffi as ffi
    whole = [torch.full((math.prod(shape) + 2 * GUARD,), PATTERN[dtype], dtype=dtype, device=device)
             for shape, dtype in outputs]
    rc = launch(*(ffi.ptr(w[GUARD:]) for w in whole))
    torch.cuda.synchronize()
    assert rc == 3
    assert ffi.load().pa_last_error().decode() == message
    for w in whole:
        assert bool((w == PATTERN[w.dtype]).all()), "a refused call wrote to its output"
