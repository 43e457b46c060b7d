"""A capture that failed must leave its stream fit for the next capture. push! synchronises, so inside a capture it invalidates
the capture; `CapturedSequence` then abandons it with a clean error. torch hands its pooled side streams out again after 32, so a
later, unrelated capture lands on the same stream: it must record and replay as on a fresh one."""
import numpy as np
import pytest
import torch

gpu = pytest.mark.gpu


@gpu
def test_a_stream_whose_capture_was_invalidated_can_be_captured_on_again(lo, dev):
    rng = np.random.default_rng(41)
    n = 1000
    to = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)        # noqa: E731
    B = lo.LBFGSOperator(n, mem=3, device=dev)
    for _ in range(3):
        s = rng.uniform(-1, 1, n)
        lo.push(B, to(s), to(s * rng.uniform(0.5, 2, n)))
    x = to(rng.uniform(-1, 1, n))
    res, ref = torch.zeros_like(x), torch.zeros_like(x)
    lo.mul(ref, B, x, 2.0, 0.0)
    side = torch.cuda.Stream(dev)
    with pytest.raises(lo.MxloError):
        with lo.CapturedSequence(dev, stream=side):
            lo.push(B, x, x * 2.0)                                          # not capturable: the capture is invalidated
    lo.mul(res, B, x, 2.0, 0.0)                                             # the ctx keeps working
    assert torch.equal(res, ref)
    g = lo.CapturedSequence(dev, stream=side)                               # the same stream again
    with g:
        lo.mul(res, B, x, 2.0, 0.0)
    res.fill_(float("nan"))
    g.replay()
    torch.cuda.synchronize()
    assert torch.equal(res, ref)
