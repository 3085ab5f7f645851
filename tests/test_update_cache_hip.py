"""GPU tests of the update step's heuristic cache end to end (`Updater(..., cache=...)`, nnet_utils.cached_heuristic_fn_dev):
with the cache on, the training triple has the same BITS as with it off, and the target network sees every distinct child row
once.  What this rests on is checked first: the closure's value of a row has the same bits in a permuted subset."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def L():
    from deepcubea_amd import _lib
    _lib.require_gpu()
    return _lib


_NETS = {}


def _closure(env_name, seed=5):
    """(env, device closure of the fp32 parity FastResnet of a small network, onehot_dtype) — built once per environment."""
    if env_name not in _NETS:
        from deepcubea_amd import _lib
        from deepcubea_amd.utils import env_utils, nnet_utils
        from deepcubea_amd.utils.pytorch_models import FastResnet, ResnetModel
        from deepcubea_amd.utils.synthetic_weights import load_synthetic_weights
        env = env_utils.get_environment(env_name)
        _, _, D, _, depth = _lib.env_ids(env_name)
        m = ResnetModel(D, depth, 256, 128, 2, 1, True)
        load_synthetic_weights(m, seed)
        fast = FastResnet(m.eval()).cuda()
        assert fast.uses_l1_kernel  # the closure takes the uint8 rows: what the cache is keyed by
        _NETS[env_name] = (env, nnet_utils.get_heuristic_fn_dev(fast, clip_zero=False, batch_size=50_000))
    return _NETS[env_name]


class Recorder:
    """A closure of the same call form that notes what it was handed (row counts, optionally the rows) and forwards."""

    def __init__(self, fn, keep_rows=False):
        self.fn, self.keep, self.sizes, self.rows = fn, keep_rows, [], []
        self.nnet = getattr(fn, "nnet", None)
        self.valid_rows = None

    def __call__(self, x, is_onehot=False):
        self.sizes.append(int(x.shape[0]))
        if self.keep:
            self.rows.append(x.detach().cpu().numpy().copy())
        return self.fn(x, is_onehot)


def _equal(a, b):
    return all(x.dtype == y.dtype and x.shape == y.shape and torch.equal(x, y) for x, y in zip(a, b)) and \
        torch.equal(a[1].view(torch.int32), b[1].view(torch.int32))  # targets: the same bits, not just equal values


def _distinct_new_per_call(calls):
    """numpy's count of the rows a perfect cache evaluates: per call, the distinct rows no earlier call has shown."""
    seen, out = set(), []
    for rows in calls:
        keys = {r.tobytes() for r in np.unique(rows, axis=0)}
        out.append(len(keys - seen))
        seen |= keys
    return out


@torch.no_grad()
@pytest.mark.parametrize("env_name", ["cube3", "puzzle15"])
def test_precondition_a_rows_value_has_the_same_bits_in_a_permuted_subset(L, env_name):
    env, hfn = _closure(env_name)
    st = L.generate_states(env._env_id, env._dim, 3000, 0, 30, 21)[0]
    x = env.expand_dev(st, children=True, nnet_in=True, solved=False, hashes=False)["nnet_in"].contiguous()
    whole = hfn(x)
    g = torch.Generator().manual_seed(1)
    for count in (1, 777, 1024, 20_001):
        p = torch.randperm(x.shape[0], generator=g)[:count].cuda()
        assert torch.equal(hfn(x[p]).view(torch.int32), whole[p].view(torch.int32)), count


@torch.no_grad()
@pytest.mark.parametrize("env_name,n,back_max,steps,eps_max", [("cube3", 4000, 30, 1, 0.0), ("cube3", 1500, 30, 3, 0.3),
                                                              ("puzzle15", 3000, 30, 1, 0.0)])
def test_gbfs_update_has_the_same_bits_and_evaluates_each_distinct_row_once(L, env_name, n, back_max, steps, eps_max):
    from deepcubea_amd.updaters.updater import Updater
    env, hfn = _closure(env_name)
    A = env.get_num_moves()
    off_rec, on_rec = Recorder(hfn, keep_rows=True), Recorder(hfn)
    kw = dict(update_batch_size=1024, eps_max=eps_max, seed=7)  # several batches: the cache lives across them
    off = Updater(env, n, back_max, off_rec, steps, "GBFS", cache="off", **kw)
    on = Updater(env, n, back_max, on_rec, steps, "GBFS", cache=1 << 20, **kw)  # >= 8 x the rows: load <= 1/8
    want = off.update_dev()
    assert off.cache_counters() is None and len(off_rec.sizes) >= -(-n // 1024) * 1
    got = on.update_dev()
    assert _equal(got, want)
    rows = sum(off_rec.sizes)
    first = (n - int(want[2].sum())) * A if steps == 1 else 0  # one step: every state that is not solved is expanded once
    assert (rows == first if steps == 1 else rows > n * A) and rows * 8 <= 1 << 20
    # the inner closure was handed exactly the distinct new rows of every call (a call with none makes no inner call)
    expect = _distinct_new_per_call(off_rec.rows)
    assert on_rec.sizes == [c for c in expect if c > 0]
    c = on.cache_counters()
    assert c["rows"] == rows and c["evaluated"] == sum(expect) and c["uncached"] == 0
    assert c["hits"] + c["dups"] + c["evaluated"] == rows and c["hits"] > 0 and c["dups"] > 0
    assert sum(expect) < rows  # fewer network rows than children
    if env_name == "cube3":
        assert sum(expect) < 0.95 * rows  # 6 of 31 scramble depths lie within five moves of the goal
    assert on.cached_fn.cache.used() == sum(expect)
    # a second run of the same Updater: the same triple again, now answered by the table alone
    before = len(on_rec.sizes)
    assert _equal(on.update_dev(), want)
    assert len(on_rec.sizes) == before and on.cache_counters()["hits"] == c["hits"] + rows
    # and the cache-off Updater repeats itself too (the comparison above is not against a moving target)
    assert _equal(off.update_dev(), want)


@torch.no_grad()
def test_astar_update_has_the_same_bits(L):
    from deepcubea_amd.updaters.updater import Updater
    env, hfn = _closure("cube3")
    on_rec, off_rec = Recorder(hfn), Recorder(hfn)
    off = Updater(env, 300, 6, off_rec, 4, "ASTAR", update_batch_size=128, seed=5, cache="off")
    on = Updater(env, 300, 6, on_rec, 4, "ASTAR", update_batch_size=128, seed=5, cache=1 << 20)
    want, got = off.update_dev(), on.update_dev()
    assert _equal(got, want) and want[0].shape[0] >= 300
    c = on.cache_counters()
    assert c["rows"] == sum(off_rec.sizes) and c["evaluated"] == sum(on_rec.sizes) < c["rows"] and c["uncached"] == 0
    assert _equal(on.update_dev(), want)


@torch.no_grad()
def test_a_closure_that_takes_onehot_rows_passes_through(L):
    from deepcubea_amd.updaters.updater import Updater
    from deepcubea_amd.utils import env_utils
    env = env_utils.get_environment("lightsout7")
    w = torch.linspace(0.25, 3.0, 49 * 6, device="cuda")

    def onehot_fn(x, is_onehot=False):
        assert is_onehot and x.shape[1] == 49 * 6
        return (x.float() * w).sum(dim=1)

    recs = [Recorder(onehot_fn), Recorder(onehot_fn)]
    off = Updater(env, 600, 6, recs[0], 1, "GBFS", update_batch_size=256, seed=2, onehot_dtype=torch.float32, cache="off")
    on = Updater(env, 600, 6, recs[1], 1, "GBFS", update_batch_size=256, seed=2, onehot_dtype=torch.float32, cache=1 << 12)
    want = off.update_dev()
    assert _equal(on.update_dev(), want)
    assert recs[0].sizes == recs[1].sizes and sum(recs[1].sizes) == (600 - int(want[2].sum())) * 49  # solved states are not expanded
    assert set(on.cache_counters().values()) == {0} and on.cached_fn.cache.used() == 0


def test_wrapper_contract_and_refusals(L):
    from deepcubea_amd.updaters.updater import Updater
    from deepcubea_amd.utils import nnet_utils
    from deepcubea_amd.utils.pytorch_models import Fp8Resnet, ResnetModel
    env, hfn = _closure("cube3")
    fn = nnet_utils.cached_heuristic_fn_dev(hfn, 54, 1 << 12)
    assert fn.cache.row_bytes == 54 and fn.cache.slots == 1 << 12 and fn.inner is hfn
    assert fn.counters() == dict(rows=0, hits=0, dups=0, evaluated=0, uncached=0)
    # empty input: straight through to the inner closure, whatever that does with it
    stub = Recorder(lambda x, is_onehot=False: torch.zeros(x.shape[0], device=x.device))
    through = nnet_utils.cached_heuristic_fn_dev(stub, 54, 64)
    assert through(torch.zeros((0, 54), dtype=torch.uint8, device="cuda")).shape == (0,)
    assert stub.sizes == [0] and through.counters()["rows"] == 0
    x = torch.randint(0, 6, (500, 54), dtype=torch.uint8, generator=torch.Generator().manual_seed(2)).cuda()
    x[250:] = x[:250]
    y = fn(x)
    assert torch.equal(y.view(torch.int32), hfn(x).view(torch.int32))
    assert fn.counters() == dict(rows=500, hits=0, dups=250, evaluated=250, uncached=0)
    assert torch.equal(fn(x[100:400]).view(torch.int32), y[100:400].view(torch.int32))
    assert fn.counters() == dict(rows=800, hits=300, dups=250, evaluated=250, uncached=0)
    # a network that calibrates on the rows it sees is refused, by the wrapper and by the Updater
    f8 = nnet_utils.get_heuristic_fn_dev(Fp8Resnet(ResnetModel(54, 6, 64, 32, 2, 1, True).eval()))
    with pytest.raises(ValueError, match="fp8"):
        nnet_utils.cached_heuristic_fn_dev(f8, 54, 1 << 12)
    with pytest.raises(ValueError, match="fp8"):
        Updater(env, 10, 5, f8, 1, cache="auto")
    assert Updater(env, 10, 5, f8, 1, cache="off").cache_spec is None
    for bad in ("on", 1000, "1e6"):
        with pytest.raises(ValueError):
            Updater(env, 10, 5, hfn, 1, cache=bad)
    # auto: sized from the shard's rows
    auto = Updater(env, 1000, 30, hfn, 1, update_batch_size=512, cache="auto")
    sn, ctg, sv = auto.update_dev()
    assert sn.shape == (1000, 54) and auto.cached_fn.cache.slots == 1 << 15 and auto.cache_counters()["rows"] == (1000 - int(sv.sum())) * 12
