"""What the native-equals-op-by-op tests of one layer Function share: ``EncoderLayerFn`` / ``PooledEncoderLayerFn`` applied directly,
once per sequencer (``XF.LAYER_CALLS`` on: one native call per pass; off: op by op through ``hip_ops``), and everything either run
leaves behind -- the saved pieces of the arena, the outputs, dx and the sixteen parameter gradients -- compared bit for bit."""
import torch

# EncoderLayerFn's parameter arguments, in order
PARAMS = ("ln1_w", "ln1_b", "wq", "bq", "wk", "bk", "wv", "bv", "wo", "bo", "ln2_w", "ln2_b", "w1", "b1", "w2", "b2")
# one weight, one bias, one LayerNorm pair, and k_proj.bias
FROZEN = ("w1", "bo", "ln2_w", "ln2_b", "bk")


def layer_params(D, Dff, seed=3):
    torch.manual_seed(seed)
    g = lambda *shape, s=0.05: torch.randn(*shape, device="cuda") * s
    vals = [1 + g(D), g(D), g(D, D), g(D), g(D, D), g(D), g(D, D), g(D), g(D, D), g(D), 1 + g(D), g(D), g(Dff, D), g(Dff), g(D, Dff), g(D)]
    return [v.requires_grad_() for v in vals]


def layer_input(B, S, D, dtype, side_rows):
    """``(x, side)``: a [B*S, D] stream in ``dtype`` and the fp32 side rows of its first ``side_rows`` tokens per sample (0: none),
    of which x holds the rounded copy"""
    x = torch.randn(B * S, D, device="cuda")
    side = None
    if side_rows:
        side = x.view(B, S, D)[:, :side_rows].reshape(B * side_rows, D).contiguous()
    return x.to(dtype).requires_grad_(), side


def run_layer(fn, native, x, params, tail, w, frozen=()):
    """One forward and backward of the Function ``fn`` (arguments: x, the 16 parameters, ``tail``) on the path ``native`` selects,
    the loss ``sum(x3 * w)``.  ``.grad`` of x and of the parameters is left as the caller set it.  Returns every result by name:
    ``piece:*`` (the saved pieces, view by view), x3, side_out, side_x2, dx and the sixteen gradients (None where frozen)."""
    import xpretrain_amd.functional as XF
    for n, p in zip(PARAMS, params):
        p.requires_grad_(n not in frozen)
    old, XF.LAYER_CALLS = XF.LAYER_CALLS, native
    try:
        out = fn.apply(x, *params, *tail)
        x3, side_out = out if isinstance(out, tuple) else (out, None)
        node = x3.grad_fn
        assert node.native == native
        saved = node.saved_tensors
        arena, side_x2 = saved[1], saved[-1]
        got = {"piece:" + n: v.clone() for n, v in XF._piece_views(node.plan, arena).items()}
        (x3.float() * w).sum().backward()
        torch.cuda.synchronize()
    finally:
        XF.LAYER_CALLS = old
    got.update(x3=x3.detach().clone(), side_out=side_out, side_x2=side_x2, dx=x.grad)
    got.update({n: p.grad for n, p in zip(PARAMS, params)})
    return got


def assert_same(a, b, frozen=()):
    """two ``run_layer`` results: the same names, None in the same places (exactly the frozen gradients among the parameters'),
    every tensor torch.equal"""
    assert list(a) == list(b)
    for n in a:
        assert (a[n] is None) == (b[n] is None), n
        if n in PARAMS:
            assert (a[n] is None) == (n in frozen), n
        if a[n] is not None:
            assert a[n].dtype == b[n].dtype and torch.equal(a[n], b[n]), f"{n} differs between the native call and the op-by-op path"


def both_paths(fn, x, params, tail, w, frozen=()):
    """``run_layer`` on either path from ``.grad is None`` everywhere; asserts they agree and returns the native result"""
    res = []
    for native in (True, False):
        for t in [x] + list(params):
            t.grad = None
        res.append(run_layer(fn, native, x, params, tail, w, frozen))
    assert_same(*res, frozen)
    return res[0]
