"""The UDF value sweep and the input-gradient sweep behind it as one launch (mlp.FUSE_SWEEPS; NUDF_CH_SEED of include/nudf.h)
against one launch per sweep: the fused launch runs the same arithmetic on the same operands, so EVERY array it leaves in
memory -- value, multiplier, features, saved activations, input-gradient adjoints, the gradient -- every parameter gradient of
the backward that reads them, and whole train steps (eager and replayed from a HIP graph) must be equal to the bit."""
import pytest
import torch

from common import build_modules, perturb_

pytestmark = pytest.mark.gpu

# 65 536: the headline launch; 19 219: ragged, 64-point tiles; 5 003: ragged, below 16 384 -> the 32-point tiles
SIZES = [65536, 19219, 5003]


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


@pytest.fixture(autouse=True)
def _default_mode():
    from neuraludf_amd import mlp
    prec, fuse = mlp.PRECISION, mlp.FUSE_SWEEPS
    mlp.set_precision("bf16x3")
    yield
    mlp.set_precision(prec)
    mlp.set_fuse_sweeps(fuse)


def _engine(dev, perturbed=True):
    """seed-0 weights; perturbed: made 'trained-like' as in the other kernel tests (the geometric initialisation zeroes the
    encoding columns of lin0 / lin4)"""
    from neuraludf_amd.models import fields
    mods = build_modules(fields, seed=0)
    if perturbed:
        mods = perturb_(mods)
    return mods["udf"].to(dev).engine()


def _points(P, dev, seed=3):
    g = torch.Generator().manual_seed(seed)
    x = (torch.rand(P, 3, generator=g) * 2 - 1).to(dev)
    # the seeded loss adjoints of tests/test_gpu_round6.py's backward tests
    d_udf = (torch.randn(P, generator=g) * 1e-4).to(dev)
    d_g = (torch.randn(P, 3, generator=g) * 1e-5).to(dev)
    d_feat = (torch.randn(P, 288, generator=g) * 1e-5).to(dev)
    return x, d_udf, d_g, d_feat


def _forward_gradient(eng, x, fuse):
    from neuraludf_amd import mlp
    mlp.set_fuse_sweeps(fuse)
    st, g, DA = eng.forward_gradient(x, feat_ld=288)
    torch.cuda.synchronize()
    return st, g, DA


def _live(t, P, width):
    """the rows and columns a sweep defines: rows >= P are tile scratch, columns >= width the allocation's padding (the saved
    arrays are not cleared, see mlp._buf)"""
    return t[:P, :width]


@pytest.mark.parametrize("perturbed", [False, True], ids=["seed0", "seed0_perturbed"])
@pytest.mark.parametrize("P", SIZES)
def test_forward_and_input_gradient_in_one_launch_leave_the_same_bits(dev, P, perturbed):
    eng = _engine(dev, perturbed)
    x = _points(P, dev)[0]
    st0, g0, DA0 = _forward_gradient(eng, x, False)
    st1, g1, DA1 = _forward_gradient(eng, x, True)
    for k in ("udf", "sign", "feat"):
        assert torch.equal(st0[k], st1[k]), k
    assert float(st0["udf"].abs().max()) > 0.0 and float(g0.abs().max()) > 0.0
    assert len(st0["X"]) == len(st1["X"]) == eng.L + 1 and len(DA0) == len(DA1) == eng.L
    for l, (a, b) in enumerate(zip(st0["X"], st1["X"])):
        assert torch.equal(_live(a, P, eng.layers[l].inp), _live(b, P, eng.layers[l].inp)), ("X", l)
    for l, (a, b) in enumerate(zip(DA0, DA1)):
        assert torch.equal(_live(a, P, eng.layers[l].out), _live(b, P, eng.layers[l].out)), ("DA", l)
    assert torch.equal(g0, g1)
    # the backward sweeps read X, sign and DA whole tiles at a time (scratch rows included): every parameter gradient
    _, d_udf, d_g, d_feat = _points(P, dev)
    grads = []
    for st, DA in ((st0, DA0), (st1, DA1)):
        grads.append([t.detach().clone() for t in eng.backward(x, st, DA, d_udf, d_feat, 288, d_g)])
    torch.cuda.synchronize()
    assert len(grads[0]) == len(grads[1]) >= 27
    for i, (a, b) in enumerate(zip(*grads)):
        assert torch.equal(a, b), ("parameter gradient", i)


def _headline_batch(dev):
    from neuraludf_amd import synth
    rays = synth.make_rays(synth.make_scene("dtu"), 0, 512, seed=1234)      # bench.py's inputs
    return {k: v.contiguous().to(dev) for k, v in rays.items()}


HEADLINE = dict(n_samples=64, n_importance=64, n_outside=0, up_sample_steps=4, perturb=1.0)


def _train(dev, fuse, graphed, n):
    from neuraludf_amd import mlp
    from neuraludf_amd.train import Trainer, GraphedStep
    mlp.set_fuse_sweeps(fuse)
    mlp._CHAIN_MEMO.clear()
    tr = Trainer(dev, HEADLINE, seed=0, fused_adam=True)
    tr.renderer.diagnostics = False
    stepper = GraphedStep(tr, eager_steps=2) if graphed else tr.step
    batch = _headline_batch(dev)
    torch.manual_seed(1234)
    losses = []
    for _ in range(n):
        loss, _ = stepper(batch)
        losses.append(loss.clone())
    torch.cuda.synchronize()
    if graphed:
        assert stepper.enabled and stepper.replays == n - 2
    return losses, [p.detach().clone() for m in tr.modules().values() for p in m.parameters()]


@pytest.mark.parametrize("graphed", [False, True], ids=["eager", "graph_replay"])
def test_train_step_on_the_benchmark_inputs_is_bit_identical(dev, graphed):
    n = 4 if graphed else 1            # graph: 2 eager steps, the capture with its first replay, one more replay
    l0, p0 = _train(dev, False, graphed, n)
    l1, p1 = _train(dev, True, graphed, n)
    for i, (a, b) in enumerate(zip(l0, l1)):
        assert torch.equal(a, b), ("loss", i, float(a), float(b))
    assert len(p0) == len(p1) > 0
    for i, (a, b) in enumerate(zip(p0, p1)):
        assert torch.equal(a, b), ("parameter", i)


def test_headline_step_has_one_chain_launch_less(dev):
    from neuraludf_amd import mlp
    from neuraludf_amd.train import Trainer
    batch = _headline_batch(dev)
    counts, labels = {}, {}
    for fuse in (False, True):
        mlp.set_fuse_sweeps(fuse)
        tr = Trainer(dev, HEADLINE, seed=0, fused_adam=True)
        tr.renderer.diagnostics = False
        torch.manual_seed(1234)
        tr.step(batch)
        mlp.PROFILE = []
        try:
            tr.step(batch)
            torch.cuda.synchronize()
            chains = [r for r in mlp.PROFILE if r[0] == "mlp_chain"]
        finally:
            mlp.PROFILE = None
        counts[fuse] = len(chains)
        labels[fuse] = [r[4] for r in chains]
    print(counts, labels[True])
    assert counts == {False: 11, True: 10}, (counts, labels)
    assert sum("udf-forward+input-gradient" in s for s in labels[True]) == 1
    assert not any("forward+input" in s for s in labels[False])


def test_the_seed_step_is_refused_out_of_place(dev):
    """SEED belongs directly behind the head of a forward sweep"""
    from neuraludf_amd import mlp
    from neuraludf_amd._lib import NudfError
    eng = _engine(dev)
    x = _points(256, dev)[0]
    st = eng.forward(x, need_grad_state=True)          # packs the weights
    torch.cuda.synchronize()
    pl = eng.layers[1]
    frag = pl.frag(mlp._kind("bwd", "grad"))
    out = torch.empty(mlp.pad_rows(256), 256, device=dev)
    cb = mlp.ChainBuilder(256, "LOAD", 256)
    cb.init_load(st["X"][2], st["X"][2].shape[1])
    cb.step("SEED", None, 256, 256, r1_col=eng.layers[eng.L].W, C1=out)          # no head in front of it
    cb.step("NONE", frag, mlp.k8(pl.out), pl.inp, C1=out, act_write=0)
    with pytest.raises(NudfError):
        cb.launch()
