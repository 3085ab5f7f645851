"""GPU tests of the heuristic cache kernels (csrc/dca_hcache.hip, include/dca.h "heuristic cache") through `_lib.HeuristicCache`
against a Python model of the table (the set of stored keys).  The "network" is an exact function f of the row computed on the
host and uploaded, so after lookup -> caller writes the EVAL rows -> finish, h[i] must equal f(row_i) for EVERY row, bit for bit.
Which of several equal rows becomes the EVAL_STORE one is left to the race: the tests assert what does not depend on it."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

HIT, EVAL_STORE, DUP, EVAL_ONLY = 0, 1, 2, 3
SENT_H, SENT_SLOT, SENT_ST = -12345.5, -77, 99
_M64 = (1 << 64) - 1


@pytest.fixture(scope="module")
def L():
    from deepcubea_amd import _lib
    _lib.require_gpu()
    return _lib


def f_of(rows: np.ndarray) -> np.ndarray:
    """An exact float32 function of the row that is NOT the table's hash: 24 bits of a multiplicative mix of the bytes."""
    k = (np.arange(rows.shape[1], dtype=np.uint64) * np.uint64(0x9E3779B1) + np.uint64(0x85EBCA77)) | np.uint64(1)
    with np.errstate(over="ignore"):
        v = (rows.astype(np.uint64) * k).sum(1, dtype=np.uint64) * np.uint64(0xD6E8FEB86659FD93)
    return (v >> np.uint64(40)).astype(np.float32)


def keys_of(rows: np.ndarray):
    return [r.tobytes() for r in rows]


def place(rows: np.ndarray, layout: str) -> torch.Tensor:
    """The rows on the device as a [n, rb] view: 'packed' = contiguous from an aligned base; 'ragged' = an odd row stride > rb inside
    a flat buffer, base offset by one row and more to an odd address, so that nothing is 16-byte aligned; 'shifted' = contiguous, base
    offset by one row (D = 54 rows then start on 2-byte boundaries)."""
    n, rb = rows.shape
    t = torch.from_numpy(rows).cuda()
    if layout == "packed":
        return t
    ld, off = ((rb + 3) | 1, (rb + 1) | 1) if layout == "ragged" else (rb, rb)  # ragged: odd stride from an odd address
    flat = torch.full((off + (n + 1) * ld + 16,), 0xEE, dtype=torch.uint8, device="cuda")
    view = flat[off:].as_strided((n, rb), (ld, 1))
    view.copy_(t)
    return view


def run_call(L, cache, view, rows, model, exact=True):
    """One lookup / evaluate / finish round, with every check that holds for any race.  `model`: set of stored keys (updated).
    exact: the table is so lightly loaded (<= 1/8) that nothing may be turned away."""
    n = rows.shape[0]
    f = f_of(rows)
    pad = 16
    h = torch.full((n + pad,), SENT_H, dtype=torch.float32, device="cuda")
    slot = torch.full((n + pad,), SENT_SLOT, dtype=torch.int32, device="cuda")
    status = torch.full((n + pad,), SENT_ST, dtype=torch.uint8, device="cuda")
    cache.lookup(view, h, slot, status)
    st, sl, hh = status.cpu().numpy(), slot.cpu().numpy(), h.cpu().numpy()
    # nothing beyond n is touched; h is written for HIT rows only
    assert (st[n:] == SENT_ST).all() and (sl[n:] == SENT_SLOT).all() and (hh[n:] == np.float32(SENT_H)).all()
    st, sl = st[:n], sl[:n]
    assert np.isin(st, (HIT, EVAL_STORE, DUP, EVAL_ONLY)).all()
    assert (hh[:n][st != HIT] == np.float32(SENT_H)).all()
    assert np.array_equal(hh[:n][st == HIT], f[st == HIT])
    assert ((sl == -1) == (st == EVAL_ONLY)).all() and (sl[st != EVAL_ONLY] >= 0).all() and (sl < cache.slots).all()
    keys = keys_of(rows)
    store_keys = [keys[i] for i in np.flatnonzero(st == EVAL_STORE)]
    assert len(set(store_keys)) == len(store_keys)            # one EVAL_STORE row per new key
    assert not (set(store_keys) & model)                      # ... and only for keys the table did not hold
    for i in np.flatnonzero(st == HIT):
        assert keys[i] in model
    for i in np.flatnonzero(st == DUP):
        assert keys[i] in set(store_keys)
    # equal rows share a slot, different stored rows never do
    by_slot = {}
    for i in np.flatnonzero(st != EVAL_ONLY):
        assert by_slot.setdefault(int(sl[i]), keys[i]) == keys[i]
    if exact:
        new = set(keys) - model
        assert int((st == EVAL_ONLY).sum()) == 0
        assert int((st == EVAL_STORE).sum()) == len(new)      # rows to evaluate == distinct new keys, exactly
        assert all(keys[i] in model for i in np.flatnonzero(st == HIT)) and int((st == HIT).sum()) == sum(k in model for k in keys)
    # the caller evaluates the EVAL rows and writes them; finish stores and fills the duplicates
    todo = torch.from_numpy(np.flatnonzero((st == EVAL_STORE) | (st == EVAL_ONLY))).cuda()
    h[todo] = torch.from_numpy(f).cuda()[todo]
    cache.finish(h, slot, status, n)
    out = h.cpu().numpy()
    assert np.array_equal(out[:n].view(np.uint32), f.view(np.uint32))  # every row, bit for bit
    assert (out[n:] == np.float32(SENT_H)).all()
    assert np.array_equal(status.cpu().numpy()[:n], st) and np.array_equal(slot.cpu().numpy()[:n], sl)  # finish reads them only
    model |= set(store_keys)
    return st


def make_rows(rng, n, rb, contents):
    rows = rng.integers(0, 256, (max(n, 1), rb), dtype=np.uint8)
    if contents == "equal":
        rows[:] = rows[0]
    elif contents == "distinct":
        rows[:, :4] = np.arange(rows.shape[0], dtype="<u4").view(np.uint8).reshape(-1, 4)
    else:  # heavy duplication: n rows drawn from n // 8 + 1 keys
        rows = rows[rng.integers(0, n // 8 + 1, rows.shape[0])]
    return np.ascontiguousarray(rows[:n])


@pytest.mark.parametrize("rb", [16, 25, 36, 49, 54, 64])
def test_lookup_finish_against_the_model(L, rb):
    rng = np.random.default_rng(rb)
    for n in (0, 1, 63, 64, 65, 4099):
        for layout, contents in (("packed", "dups"), ("ragged", "distinct"), ("shifted", "equal"), ("ragged", "dups"),
                                 ("shifted", "distinct")):
            cache = L.HeuristicCache(rb, 1 << 16)  # <= 2 x 4099 keys: load <= 1/8
            model = set()
            rows = make_rows(rng, n, rb, contents)
            view = place(rows, layout)
            if layout == "ragged" and n > 1:
                assert view.data_ptr() % 2 == 1 and view.stride(0) % 2 == 1 and view.stride(0) > rb
            st = run_call(L, cache, view, rows, model)
            assert cache.used() == len(model) == len(set(keys_of(rows)))
            assert int((st == HIT).sum()) == 0
            # a second call with the same rows (another layout): all HIT, nothing new
            st2 = run_call(L, cache, place(rows, "packed" if layout != "packed" else "ragged"), rows, model)
            assert (st2 == HIT).all() and cache.used() == len(model)
            # a third with half old, half new rows
            if n >= 63:
                more = make_rows(rng, n, rb, "distinct")
                more[:, 4] ^= 0xFF
                mixed = np.ascontiguousarray(np.concatenate((rows[: n // 2], more[: n - n // 2]))[rng.permutation(n)])
                st3 = run_call(L, cache, place(mixed, layout), mixed, model)
                assert int((st3 == HIT).sum()) >= n // 2 and cache.used() == len(model)


def test_grid_stride_loop_covers_a_large_n(L):
    """More rows than the largest grid has threads (8192 blocks x 256): the tail is reached by the grid-stride loop."""
    rng = np.random.default_rng(7)
    n = 8192 * 256 + 77
    pool = make_rows(rng, 1000, 16, "distinct")
    rows = np.ascontiguousarray(pool[rng.integers(0, 1000, n)])
    rows[-1] = 0xAB  # a key that only the very last row has
    cache = L.HeuristicCache(16, 1 << 22)
    t = torch.from_numpy(rows).cuda()
    f = torch.from_numpy(f_of(rows)).cuda()
    h, slot, status = cache.lookup(t)
    todo = ((status == EVAL_STORE) | (status == EVAL_ONLY)).nonzero().view(-1)
    assert todo.numel() == 1001 and int((status == EVAL_ONLY).sum()) == 0 and int(status[-1]) == EVAL_STORE
    h[todo] = f[todo]
    cache.finish(h, slot, status)
    assert torch.equal(h, f) and cache.used() == 1001
    h2, _, status2 = cache.lookup(t)
    assert bool((status2 == HIT).all()) and torch.equal(h2, f)


def test_fill_limit_holds_and_the_rest_is_eval_only(L):
    rng = np.random.default_rng(11)
    rows = make_rows(rng, 1000, 16, "distinct")
    cache = L.HeuristicCache(16, 64)
    model = set()
    st = run_call(L, cache, place(rows, "packed"), rows, model, exact=False)
    stored = int((st == EVAL_STORE).sum())
    assert 1 <= stored <= 32 and cache.used() == stored == len(model)      # no slot is claimed once slots / 2 are in use
    assert int((st == EVAL_ONLY).sum()) == 1000 - stored and not ((st == HIT) | (st == DUP)).any()
    # afterwards the table answers what it holds; every value is still right (run_call checks all 1000)
    for _ in range(3):
        before = set(model)
        st = run_call(L, cache, place(rows, "ragged"), rows, model, exact=False)
        assert all((k in before) == (s == HIT) for k, s in zip(keys_of(rows), st))
        assert cache.used() == len(model) <= 32
    # clear empties it
    cache.clear()
    assert cache.used() == 0
    st = run_call(L, cache, place(rows[:8], "packed"), rows[:8], set())
    assert (st == EVAL_STORE).all()


def _hash_state_after_word0(w0: int, d: int) -> int:
    """oracle.np_oracle.hash64's arithmetic up to and including the first word."""
    h = (0x9E3779B97F4A7C15 ^ ((d * 0xD6E8FEB86659FD93) & _M64)) & _M64
    h ^= w0
    h = (h * 0xFF51AFD7ED558CCD) & _M64
    h ^= h >> 32
    return h


def test_true_hash_collisions_keep_their_own_values(L):
    """The hash mixes one 8-byte word at a time: two 16-byte rows with different first words collide when the second word of one
    is w1 ^ s0 ^ s0' (s0, s0' the states after word 0).  Equality is the bytes, not the hash."""
    from oracle import np_oracle as no
    rng = np.random.default_rng(5)
    pairs = []
    for _ in range(8):
        a0, a1, b0 = (int(x) for x in rng.integers(0, 1 << 63, 3, dtype=np.uint64))
        b1 = a1 ^ _hash_state_after_word0(a0, 16) ^ _hash_state_after_word0(b0, 16)
        pairs.append(np.array([[a0, a1], [b0, b1]], dtype="<u8").view(np.uint8).reshape(2, 16))
    for pair in pairs:
        ho = no.hash64(pair)
        hd = L.hash64(torch.from_numpy(pair).cuda()).cpu().numpy().view(np.uint64)
        assert ho[0] == ho[1] and np.array_equal(ho, hd) and not np.array_equal(pair[0], pair[1])
        assert f_of(pair)[0] != f_of(pair)[1]
        cache = L.HeuristicCache(16, 1 << 10)
        model = set()
        a, b = pair[:1].copy(), pair[1:].copy()
        assert run_call(L, cache, place(a, "packed"), a, model, exact=False).tolist() == [EVAL_STORE]
        assert run_call(L, cache, place(b, "shifted"), b, model, exact=False).tolist() == [EVAL_ONLY]  # same tag, other bytes
        both = np.ascontiguousarray(np.concatenate((pair, pair[::-1])))
        assert run_call(L, cache, place(both, "ragged"), both, model, exact=False).tolist() == [HIT, EVAL_ONLY, EVAL_ONLY, HIT]
        assert cache.used() == 1
        # both in ONE call of an empty table: one of them is stored, the other evaluated on its own; each gets its own value
        fresh = L.HeuristicCache(16, 1 << 10)
        st = run_call(L, fresh, place(pair, "packed"), pair, set(), exact=False)
        assert sorted(st.tolist()) == [EVAL_STORE, EVAL_ONLY]


def test_a_claim_that_never_stored_is_not_shared(L):
    """A key claimed by a call whose caller never called finish has no value: later calls evaluate it and store nothing."""
    rng = np.random.default_rng(3)
    rows = make_rows(rng, 300, 54, "dups")
    cache = L.HeuristicCache(54, 1 << 12)
    _, _, status = cache.lookup(torch.from_numpy(rows).cuda())
    assert int((status == EVAL_STORE).sum()) == len(set(keys_of(rows)))
    st = run_call(L, cache, place(rows, "shifted"), rows, set(), exact=False)
    assert (st == EVAL_ONLY).all()
    # and the wrapper refuses rows of another width or type before any launch
    with pytest.raises(ValueError):
        cache.lookup(torch.zeros((4, 16), dtype=torch.uint8, device="cuda"))
    with pytest.raises(ValueError):
        cache.lookup(torch.zeros((4, 54), dtype=torch.float32, device="cuda"))
