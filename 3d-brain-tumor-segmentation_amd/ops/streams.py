"""The step fence and the side streams of a training step (host side only: no library call is made here)."""
import torch

_side = {}
_side_enabled = True
_fence = {}


def step_fence(kind='train', depth=2):
    """Bound how far the host runs ahead of the GPU: call at the START of a step -- waits (host side) until the step issued `depth`
    calls earlier has finished, then notes this one.  A step enqueues in 2-12 ms what the GPU runs in 7-80 ms; left unbounded, the
    host gets many steps ahead, every one of them holding its activations (blocks freed on a side stream cannot be handed out again
    before that stream's work has run), the caching allocator answers with new hipMalloc segments inside the timed region -- the
    reserved pool was seen to grow from 100 to 140 GB for 42 GB of live tensors, and steps to take 120-400 ms instead of 79.  With
    at most `depth` steps in flight the allocation pattern is the same every step.  BTS_STEP_FENCE=0 disables it (A/B)."""
    import os
    if not torch.cuda.is_available() or os.environ.get('BTS_STEP_FENCE') == '0':
        return
    key = (torch.cuda.current_device(), kind)
    q = _fence.setdefault(key, [])
    while len(q) >= depth:
        q.pop(0).synchronize()
    ev = torch.cuda.Event()
    q.append(ev)
    return ev


def step_fence_done(ev):
    """call at the END of the step with what step_fence returned: the event is recorded behind everything the step enqueued on the
    current stream (side streams are joined before a step returns)"""
    if ev is not None:
        ev.record(torch.cuda.current_stream())


def enable_side_streams(on):
    """switch the extra streams off / on at run time (bench.py measures per-kernel launch durations with one stream: a kernel
    that shares the chip with another stream's kernels has no launch duration of its own)"""
    global _side_enabled
    join_side_stream()
    _side_enabled = bool(on)


def side_stream(which='wgrad'):
    """Extra HIP streams of a training step (one process still drives one GPU):
      'wgrad'  the weight gradients (a third of the step, needed only by the optimiser) run there while the data-gradient
               chain -- with its many short normalisation / gate kernels that leave most CUs idle -- keeps the main stream;
      'gate'   a ResNet block's shortcut / squeeze-excitation branch (HBM-bound 1x1x1 conv, pooling, tiny MLP and their
               gradients: resnet.py:118-130) next to its conv branch (matrix-pipe-bound), joined where the two meet.
    BTS_WGRAD_STREAM=0 / BTS_GATE_STREAM=0 put the respective work back on the main stream (A/B aids)."""
    import os
    if not _side_enabled or not torch.cuda.is_available() or os.environ.get('BTS_%s_STREAM' % which.upper()) == '0':
        return None
    key = (torch.cuda.current_device(), which)
    s = _side.get(key)
    if s is None:
        s = torch.cuda.Stream(device=key[0])
        _side[key] = s
    return s


def join_side_stream():
    """the current stream waits for everything enqueued on the side streams so far (before the regulariser / the gradient
    exchange / the optimiser touch the parameter gradients)"""
    if not torch.cuda.is_available():
        return
    dev = torch.cuda.current_device()
    for (d, _), s in _side.items():
        if d == dev:
            torch.cuda.current_stream().wait_stream(s)


def wait_side_stream_event(which='wgrad'):
    """the current stream waits for what side stream `which` holds at this moment (an event recorded there now); later launches on
    the side stream are not waited for.  A gloo group drains the producing stream on the host instead (parallel._sum_over_ranks)."""
    if not torch.cuda.is_available():
        return
    s = _side.get((torch.cuda.current_device(), which))
    if s is None:
        return
    ev = torch.cuda.Event()
    ev.record(s)
    torch.cuda.current_stream().wait_event(ev)
