"""The host side of the optimiser table (train.load_optim, train.NaSGD / NaRMSprop / NaAdam / NaAdamW, ops.optim_step) without a GPU:
what load_optim builds per --opt-kind, the fallback to torch's own step on tensors the kernel does not fit, state_dict interchange,
step hooks, and that a refused kernel call leaves the optimiser as it was."""
import types

import pytest
import torch

import nerf_atlas_amd.train as T
from nerf_atlas_amd import ops

KINDS = {"adam": (T.NaAdam, torch.optim.Adam), "sgd": (T.NaSGD, torch.optim.SGD), "adamw": (T.NaAdamW, torch.optim.AdamW),
         "rmsprop": (T.NaRMSprop, torch.optim.RMSprop)}


def ns(kind, lr=1e-2, decay=0.0):
    return types.SimpleNamespace(opt_kind=kind, learning_rate=lr, decay=decay)


def params(seed=0):
    torch.manual_seed(seed)
    return [torch.nn.Parameter(torch.randn(*s)) for s in ((5, 3), (7,), (1,))]


def set_grads(a, b, step):
    torch.manual_seed(100 + step)
    for p, q in zip(a, b):
        g = torch.randn(p.shape)
        p.grad, q.grad = g, g.clone()


@pytest.mark.parametrize("kind", sorted(KINDS))
def test_load_optim_builds_the_references_table(kind, monkeypatch):
    monkeypatch.delenv("NA_OPTIM", raising=False)
    monkeypatch.delenv("NA_ADAM", raising=False)
    opt = T.load_optim(ns(kind, lr=3e-3, decay=0.25), params())
    assert type(opt) is KINDS[kind][0] and isinstance(opt, KINDS[kind][1])
    d = opt.defaults
    assert d["lr"] == 3e-3
    assert ("eps" not in d) if kind == "sgd" else d["eps"] == 1e-7
    assert d["weight_decay"] == {"adam": 0.25, "adamw": 1e-2, "sgd": 0, "rmsprop": 0}[kind]   # --decay reaches adam only
    if kind == "adamw":
        assert d["decoupled_weight_decay"] is True
    if kind in ("sgd", "rmsprop"):
        assert d["momentum"] == 0
    # generators are accepted, like model.parameters()
    assert len(T.load_optim(ns(kind), iter(params())).param_groups[0]["params"]) == 3


def test_torchs_classes_on_request(monkeypatch):
    monkeypatch.delenv("NA_ADAM", raising=False)
    monkeypatch.setenv("NA_OPTIM", "torch")
    for kind, (_, cls) in KINDS.items():
        assert type(T.load_optim(ns(kind), params())) is cls
    monkeypatch.delenv("NA_OPTIM")
    monkeypatch.setenv("NA_ADAM", "torch")
    assert type(T.load_optim(ns("adam"), params())) is torch.optim.Adam
    assert type(T.load_optim(ns("rmsprop"), params())) is T.NaRMSprop


def test_uniform_adam_and_unknown_kinds_raise():
    with pytest.raises(NotImplementedError, match="cdist"):
        T.load_optim(ns("uniform_adam"), params())
    with pytest.raises(NotImplementedError, match="unknown opt kind lion"):
        T.load_optim(ns("lion"), params())


@pytest.mark.parametrize("kind", sorted(KINDS))
def test_host_tensors_take_torchs_step_and_hooks_fire_once(kind, monkeypatch):
    """on host tensors every class is torch's class: the same parameters and state after every step, the kernel entry never called, a
    step hook fired once per step, and the state_dict loads into torch's class and back"""
    monkeypatch.setattr(ops, "optim_step", lambda *a, **k: pytest.fail("the kernel entry was called for host tensors"))
    cls, torch_cls = KINDS[kind]
    torch_cls(params(), lr=1e-2).register_step_post_hook(lambda *a: None)   # (torch's class has been instantiated: its step is hooked)
    a, b = params(), params()
    oa, ob = T.load_optim(ns(kind, decay=0.01), a), torch_cls(b, **{k: v for k, v in dict(lr=1e-2, eps=1e-7).items() if kind != "sgd" or k == "lr"},
                                                              **({"weight_decay": 0.01} if kind == "adam" else {}))
    fired = []
    oa.register_step_pre_hook(lambda *x: fired.append("pre"))
    oa.register_step_post_hook(lambda *x: fired.append("post"))
    for step in range(4):
        set_grads(a, b, step)
        oa.step()
        ob.step()
        assert all(torch.equal(p, q) for p, q in zip(a, b))
        assert all(sorted(oa.state[p]) == sorted(ob.state[q]) and all(torch.equal(oa.state[p][k], ob.state[q][k]) for k in oa.state[p])
                   for p, q in zip(a, b))
    assert fired == ["pre", "post"] * 4
    fresh_torch, fresh_mine = torch_cls(params(1), lr=1e-2), cls(params(1), lr=1e-2)
    fresh_torch.load_state_dict(oa.state_dict())
    fresh_mine.load_state_dict(ob.state_dict())
    assert sorted(fresh_mine.state_dict()["state"]) == sorted(oa.state_dict()["state"])
    for x, y in zip(fresh_mine.state_dict()["state"].values(), oa.state_dict()["state"].values()):
        assert sorted(x) == sorted(y) and all(torch.equal(torch.as_tensor(x[k]), torch.as_tensor(y[k])) for k in x)


@pytest.mark.parametrize("kind,unfit", [("sgd", dict(momentum=0.9)), ("sgd", dict(nesterov=True, momentum=0.5)), ("sgd", dict(maximize=True)),
                                         ("rmsprop", dict(centered=True)), ("rmsprop", dict(momentum=0.5)), ("adam", dict(amsgrad=True)),
                                         ("adam", dict(betas=(0.4, 0.999))), ("adamw", dict(capturable=True)),
                                         ("adam", dict(lr=torch.tensor(1e-2)))])
def test_what_the_kernel_does_not_fit(kind, unfit):
    """the gate itself (on a GPU such a group takes torch's step; tests/test_gpu_optim.py runs two of them)"""
    cls = KINDS[kind][0]
    assert cls(params(), **{"lr": 1e-2, **unfit})._fits(cls(params(), **{"lr": 1e-2, **unfit}).param_groups[0]) is False
    assert cls(params(), lr=1e-2)._fits(cls(params(), lr=1e-2).param_groups[0]) is True


@pytest.mark.parametrize("kind", ["adam", "adamw", "rmsprop"])   # (sgd keeps no state)
def test_a_refused_kernel_call_leaves_the_optimiser_as_it_was(kind, monkeypatch):
    """the tensors are validated before any state is created or counted: with both gates forced open on host tensors, ops.optim_step's
    checks refuse the state tensors -- no state appears for a new parameter, and existing step counts and moments stay"""
    cls = KINDS[kind][0]
    a = params()
    opt = cls(a, lr=1e-2)
    set_grads(a, params(), 0)
    opt.step()   # torch's step: state exists now
    fresh = torch.nn.Parameter(torch.randn(3))
    fresh.grad = torch.randn(3)
    opt.param_groups[0]["params"].append(fresh)
    before = {k: {n: torch.as_tensor(v).clone() for n, v in st.items()} for k, st in opt.state_dict()["state"].items()}
    kept = [p.detach().clone() for p in a]
    monkeypatch.setattr(cls, "_fits", lambda self, group: True)
    monkeypatch.setattr(cls, "_tensors_fit", staticmethod(lambda ps, grads: True))
    monkeypatch.setattr(ops, "optim_step", lambda *x, **k: pytest.fail("launched after a failed check"))
    with pytest.raises(ValueError, match="contiguous fp32 device tensors only"):
        opt.step()
    after = opt.state_dict()["state"]
    assert sorted(after) == sorted(before) and fresh not in opt.state
    assert all(torch.equal(torch.as_tensor(after[k][n]), before[k][n]) for k in before for n in before[k])
    assert all(torch.equal(p, q) for p, q in zip(a, kept))
    assert all(float(opt.state[p]["step"]) == 1 for p in a)


def test_step_counts_advance_together_and_survive_a_loaded_state():
    """_count_steps: one host operation per group; a state that changed underneath (a loaded state_dict, a new parameter) is noticed"""
    a, b = params(), params()
    opt, ref = T.NaRMSprop(a, lr=1e-2), torch.optim.RMSprop(b, lr=1e-2)
    set_grads(a, b, 0)
    opt.step()
    ref.step()
    group = opt.param_groups[0]
    assert opt._count_steps(group, a) == [2.0] * 3 and opt._count_steps(group, a) == [3.0] * 3
    assert all(opt.state[p]["step"].shape == () and opt.state[p]["step"].dtype == ref.state[q]["step"].dtype and float(opt.state[p]["step"]) == 3
               for p, q in zip(a, b))
    opt.load_state_dict(ref.state_dict())
    group = opt.param_groups[0]
    assert opt._count_steps(group, a) == [2.0] * 3
    opt.state[a[1]]["step"] = torch.tensor(7.0)
    assert opt._count_steps(group, a) == [3.0, 8.0, 3.0] and [float(opt.state[p]["step"]) for p in a] == [3.0, 8.0, 3.0]
    assert opt._count_steps(group, a[:2]) == [4.0, 9.0] and float(opt.state[a[2]]["step"]) == 3.0


def test_optim_step_argument_checks():
    p = [torch.zeros(4)]
    with pytest.raises(ValueError, match="unknown update rule"):
        ops.optim_step("lion", p, p, [], [], [0.0], 0)
    with pytest.raises(ValueError, match="one length"):
        ops.optim_step("rmsprop", p, p, [], [], [0.0] * 4, 0)
    with pytest.raises(ValueError, match="one length"):
        ops.optim_step("sgd", p, p, p, [], [0.0], 0)
    with pytest.raises(ValueError, match="device tensors only"):
        ops.optim_step("sgd", p, p, [], [], [0.0], 0)
