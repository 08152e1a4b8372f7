#!/usr/bin/env python3
"""Worker of tests/test_gpu_surface.py (a fresh process: torch's GPU state stays out of the pytest process; one GPU).

A context is built on a non-default torch.cuda.Stream.  On that stream a torch kernel writes the texels, upload_block_device is enqueued
behind it without a host synchronisation, and Volume.surface follows: its mesh must equal the statement's on the uploaded texels.  Then
Surface.device_tensors: the handle's own buffers as torch tensors hold the same words.  Prints PASS and exits 0."""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)


def main():
    import numpy as np
    import torch
    import vpt_amd
    from vpt_amd.surface import surface_texels

    dev = torch.device('cuda', 0)
    stream = torch.cuda.Stream(device=dev)
    ctx = vpt_amd.Context(0, stream=stream.cuda_stream)
    d, h, w = 7, 9, 37
    texels = np.random.default_rng(31).integers(0, 256, (d, h, w), dtype=np.uint8)
    vol = vpt_amd.Volume.from_array(ctx, np.zeros((d, h, w), np.uint8))
    host = torch.from_numpy(texels.astype(np.int32))
    with torch.cuda.stream(stream):
        src = (host.to(dev, non_blocking=False) + 0).to(torch.uint8)        # produced on the caller's stream
        vol.upload_block_device(0, 0, 0, w, h, d, src.data_ptr(), src.numel())
        s = vol.surface(128)
        tv, tq = s.device_tensors()
        got_v, got_q = tv.cpu().numpy().view(np.uint32), tq.cpu().numpy().view(np.uint32)
    wv, wq = surface_texels(texels, 128)
    assert len(wv) > 1000
    assert np.array_equal(s.vertices(), wv) and np.array_equal(s.quads(), wq), 'the surface is not that of the uploaded texels'
    assert got_v.shape == wv.shape and np.array_equal(got_v, wv) and np.array_equal(got_q, wq), 'device tensors differ'
    s.destroy(); vol.destroy()
    torch.cuda.synchronize()
    ctx.destroy()
    print('PASS')


if __name__ == '__main__':
    main()
