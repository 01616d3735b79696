"""Run by tests/test_feature_distance.py::test_stream_and_graph_replay_in_a_child_process in a process of its own (a capture that
goes wrong takes the process down inside hipStreamEndCapture — the suite must survive that and report it).

1. Stream order: the features are produced on a side stream by a chain of operators long enough to still be running when the
   distance is enqueued; the distance, enqueued inside the same ``torch.cuda.stream`` block, must wait for them.
2. Capture and replay of forward + backward in a single-stream ``torch.cuda.graph`` equals the eager step bit for bit (the
   operator has no atomics), also after the inputs were overwritten in place between replays."""
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main():
    from planedepth_amd import ops
    g = torch.Generator().manual_seed(31)
    shapes = [(2, 64, 24, 80), (2, 128, 12, 40), (2, 256, 6, 20)]
    target = [torch.randn(s, generator=g).cuda() for s in shapes]
    noise_p = [0.3 * torch.randn(s, generator=g).cuda() for s in shapes]
    noise_s = [0.3 * torch.randn(s, generator=g).cuda() for s in shapes]
    torch.cuda.synchronize()

    # 1. a side stream's producer is waited for
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        a = torch.randn(2048, 2048, device="cuda")
        for _ in range(40):       # ~ milliseconds of work queued ahead of the features on this stream
            a = (a @ a).tanh()
        bump = a[0, 0] * 0.0      # a device scalar that exists only once the chain has run
        pred = [(t + n + bump).requires_grad_(True) for t, n in zip(target, noise_p)]
        source = [t + n + bump for t, n in zip(target, noise_s)]
        loss = ops.feature_distance(pred, target, source)
        grads = torch.autograd.grad(loss, pred)
    side.synchronize()
    torch.cuda.synchronize()
    want = ops.feature_distance([p.detach() for p in pred], target, source)
    torch.cuda.synchronize()
    assert torch.isfinite(loss) and float(loss) > 0 and torch.equal(loss, want), (float(loss), float(want))
    assert all(float(x.abs().max()) > 0 for x in grads)

    # 2. capture and replay
    pred = [(t + n).requires_grad_(True) for t, n in zip(target, noise_p)]
    source = [t + n for t, n in zip(target, noise_s)]
    keep = {}

    def step():
        for p in pred:
            p.grad = None
        out = ops.feature_distance(pred, target, source)
        out.backward()
        keep.update(loss=out, **{"g%d" % i: p.grad for i, p in enumerate(pred)})

    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):   # (the warm-up torch documents for captures with a backward)
        for _ in range(3):
            step()
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        step()
    for round_ in range(2):
        for _ in range(2):
            graph.replay()
        torch.cuda.synchronize()
        got = {k: v.detach().clone() for k, v in keep.items()}
        with torch.no_grad():
            eager_pred = [p.detach().clone().requires_grad_(True) for p in pred]
        out = ops.feature_distance(eager_pred, target, source)
        out.backward()
        torch.cuda.synchronize()
        assert torch.equal(got["loss"], out.detach()), (round_, float(got["loss"]), float(out))
        for i, p in enumerate(eager_pred):
            share = float((p.grad != 0).double().mean())
            assert 0.05 < share < 0.95, (round_, i, share)      # both branches of the min are taken at every level
            assert torch.equal(got["g%d" % i], p.grad), (round_, i)
        if round_ == 0:
            first = got
        else:
            assert not torch.equal(got["loss"], first["loss"]) and not torch.equal(got["g1"], first["g1"])
        with torch.no_grad():       # new values in the captured buffers (both distances shrink, so the min still takes both
            for p, t in zip(pred, target):   # branches): the next replays must see them
                p.lerp_(t, 0.03)
            source[0].lerp_(target[0], 0.05)
        torch.cuda.synchronize()
    print("stream and graph replay: ok")


if __name__ == "__main__":
    main()
