"""The invariant checkers' specification, and the failing batches the checker tests run on.

Specification.  `spec_single_mask` / `spec_multi_mask` restate the reference's checks for ONE env (wurm/utils.py:113-178
`snake_consistency` / `env_consistency`; wurm/envs/multi_snake.py:733-769 `MultiSnake.check_consistency`) in numpy and
float64, and return the bit of EVERY failing check, where the reference raises on the first.  They are written from the
reference's text alone: this module's top level imports numpy and nothing else, and the specification calls neither the
oracle nor a kernel — it is what both are compared with (tests/test_checker_batches_cpu.py pins it to the reference's
recorded verdicts first).

Cases.  `single_batch` / `multi_batch` start from valid states — the oracle's reset and a few of its steps (the only
place the oracle is used here, imported inside `_valid_*`), or snakes laid by hand where a state has to have a cell free
or the snake in a chosen place — and give every env one corruption KIND at one POSITION.  The checkers do not know the
border from any other cell, so a hand-laid snake may lie anywhere.  Every head and body value written is an integer, every
food value 0, 1 or 2 (the generator's `food_value_half` stays with the fixtures: its place here is `food_value_2_elsewhere`).
`needle` gives a batch that is valid everywhere but in one env."""
import numpy as np

(FOOD_VALUE, ONE_HEAD, HAS_SNAKE, HEAD_AT_END, BODY_RANGE, MIN_LENGTH, HEAD_ON_FOOD, ONE_FOOD) = (1 << i for i in range(8))
OVERLAP, DEAD_NONZERO = 0x100, 0x200
SINGLE_BITS = (FOOD_VALUE, ONE_HEAD, HAS_SNAKE, HEAD_AT_END, BODY_RANGE, MIN_LENGTH, HEAD_ON_FOOD, ONE_FOOD)
MULTI_BITS = SINGLE_BITS[:7] + (OVERLAP, DEAD_NONZERO)
EPS = np.float32(1e-6)  # the reference's config.EPS, compared in fp32 as its `.gt(EPS)` does


# ------------------------------------------------------------------------------------------------ the specification

def _snake_mask(f, h, b):
    """snake_consistency (wurm/utils.py:113-164) of one env's planes, float64"""
    m = 0
    if not np.all((f == 0) | (f == 1)):
        m |= FOOD_VALUE
    hs, bs, bm, hb, hf = h.sum(), b.sum(), b.max(), (h * b).sum(), (h * f).sum()
    if hs != 1:
        m |= ONE_HEAD
    if not bs > 0:
        m |= HAS_SNAKE
    if bm != hb:
        m |= HEAD_AT_END
    if (np.sqrt(8 * bs + 1) - 1) / 2 != bm:   # the body sum is the bm-th triangular number
        m |= BODY_RANGE
    if not bs >= 6:
        m |= MIN_LENGTH
    if hf != 0:
        m |= HEAD_ON_FOOD
    return m


def spec_single_mask(env) -> int:
    """env_consistency (wurm/utils.py:167-178) of one (3, S, S) env: the bits of every failing check"""
    e = np.asarray(env, np.float64)
    e = e.reshape(3, -1) if e.ndim == 3 else e.reshape(e.shape[-3], -1)
    assert e.shape[0] == 3
    m = _snake_mask(e[0], e[1], e[2])
    if e[0].sum() != 1:
        m |= ONE_FOOD
    return m


def spec_multi_mask(foods, heads, bodies, dones) -> int:
    """MultiSnake.check_consistency (multi_snake.py:733-769) of one env: foods (S, S), heads / bodies (K, S, S) (any
    shape with those element counts), dones (K).  As there: the living snakes' planes are ROUNDED (half to even, like
    torch.round) before snake_consistency sees them, with the env's food plane — so the food-value bit needs a living
    snake —, the overlap count is of raw body values above EPS, and a dead snake must only be all zeros."""
    d = np.asarray(dones).reshape(-1) != 0
    K = d.size
    f = np.asarray(foods, np.float64).reshape(-1)
    h, b = np.asarray(heads, np.float64).reshape(K, -1), np.asarray(bodies, np.float64).reshape(K, -1)
    assert h.shape[1] == f.size and b.shape == h.shape
    m = 0
    for s in range(K):
        if d[s]:
            if (h[s].sum() + b[s].sum()) != 0:
                m |= DEAD_NONZERO
        else:
            m |= _snake_mask(np.rint(f), np.rint(h[s]), np.rint(b[s]))
    if ((np.asarray(bodies, np.float32).reshape(K, -1) > EPS).sum(axis=0).max()) > 1:
        m |= OVERLAP
    return m


def spec_single_masks(envs):
    return np.array([spec_single_mask(e) for e in envs], np.uint32)


def spec_multi_masks(st):
    N = st['foods'].shape[0]
    K = st['heads'].shape[0] // N
    h, b, d = st['heads'].reshape(N, K, -1), st['bodies'].reshape(N, K, -1), st['dones'].reshape(N, K)
    return np.array([spec_multi_mask(st['foods'][i], h[i], b[i], d[i]) for i in range(N)], np.uint32)


# ------------------------------------------------------------------------------------------------ positions

def tail_start(C: int) -> int:
    """first cell of the last group of 64 (the group a per-lane validity mask cuts)"""
    return ((C - 1) // 64) * 64


def cell_list(C: int, multi: bool = False):
    """where a corruption that ADDS a cell may put it: both ends of the first group of 64, the start of the second, the
    last multiple of 64 below C and the cell before it, the last cell — and for MultiSnake the first cell of a snake's
    second and third item of 11 rows of 64 cells"""
    last64 = ((C - 1) // 64) * 64
    cells = [0, 63, 64, last64 - 1, last64, C - 1] + ([64 * 11, 64 * 22] if multi else [])
    out = []
    for c in cells:
        if 0 <= c < C and c not in out:
            out.append(c)
    return out


# ------------------------------------------------------------------------------------------------ valid states

def _lay_single(e, S, rng, avoid=(), tail=False, length=None):
    """a snake (tail 1 .. head L, on consecutive cells) and one food laid by hand into the cleared (3, C) env; with
    `tail` all of it inside the last group of 64 cells"""
    C = S * S
    e[...] = 0
    lo = tail_start(C) if tail else 0
    L = length or int(rng.randint(3, 6))
    L = min(L, C - lo - 2)
    starts = [p for p in range(lo, C - L + 1) if not any(p <= c < p + L for c in avoid)]
    assert L >= 3 and starts, (S, tail, avoid)
    p = starts[int(rng.randint(len(starts)))]
    cells = list(range(p, p + L))
    if rng.randint(2):
        cells = cells[::-1]
    for v, c in enumerate(cells):
        e[2, c] = v + 1
    e[1, cells[-1]] = 1
    free = [c for c in range(lo, C) if not p <= c < p + L and c not in avoid]
    assert free, (S, tail)
    e[0, free[int(rng.randint(len(free)))]] = 1


def _valid_single(S, N, seed):
    """(N, 3, S, S) valid envs: the oracle's reset and ten of its steps with resets where it builds envs of the size,
    hand-laid ones below that (the reference builds none below 9 x 9... nor does the oracle)"""
    rng = np.random.RandomState(1000 + seed)
    envs = np.zeros((N, 3, S, S), np.float32)
    if S >= 9:
        from oracle import oracle as _o
        _o.single_reset(envs, np.ones(N), 'none', seed=seed, call=0)
        for t in range(10):
            _, _, done, _, _ = _o.single_step(envs, rng.randint(0, 4, size=N).astype(np.int64), 'none', seed=seed, call=1 + 2 * t)
            _o.single_reset(envs, done, 'none', seed=seed, call=2 + 2 * t)
    else:
        for i in range(N):
            _lay_single(envs[i].reshape(3, -1), S, rng)
    return envs


def _lay_multi(f, h, b, d, S, rng, avoid=(), tail=False):
    """K living length-3 snakes and one food laid by hand into the cleared env, each snake in a slot of three consecutive
    cells (slots start every four cells); with `tail` snake 0 and snake K - 1 get the last two slots, inside the last
    group of 64 cells, and the food lies there too"""
    K, C = h.shape
    f[...] = 0; h[...] = 0; b[...] = 0; d[...] = 0
    slots = [p for p in range(0, C - 2, 4) if not any(p <= c < p + 3 for c in avoid)]
    assert len(slots) >= K, (K, S)
    pick = [slots[j] for j in rng.choice(len(slots) - (2 if tail else 0), size=K, replace=False)]
    if tail:
        assert slots[-2] >= tail_start(C), (K, S)
        pick[0] = slots[-1]
        if K > 1:
            pick[K - 1] = slots[-2]
    used = set()
    for s, p in enumerate(pick):
        cells = list(range(p, p + 3))
        if rng.randint(2):
            cells = cells[::-1]
        for v, c in enumerate(cells):
            b[s, c] = v + 1
        h[s, cells[-1]] = 1
        used.update(cells)
    free = [c for c in range(tail_start(C) if tail else 0, C) if c not in used and c not in avoid]
    assert free, (K, S)
    f[free[int(rng.randint(len(free)))]] = 1


def _valid_multi(K, S, N, seed):
    """a MultiSnake state dict of N valid envs: the oracle's reset and four of its steps with resets (snakes die and
    are cleared on the way: mixed dones), hand-laid envs where the oracle cannot place every snake"""
    from oracle import oracle as _o
    rng = np.random.RandomState(2000 + seed)
    st = _o.multi_empty_state(N, K, S)
    cfg = _o.multi_cfg(K)
    placed = False
    if K * 12 <= (S - 2) * (S - 2) and K <= 16:
        placed = _o.multi_reset(st, np.ones(N), cfg, seed=seed, call=0) == 0
        for t in range(4 if placed else 0):
            out = _o.multi_step(st, rng.randint(0, 4, size=(K, N)), cfg, 'none', seed=seed, call=1 + 2 * t)
            placed = _o.multi_reset(st, out['all_done'], cfg, seed=seed, call=2 + 2 * t) == 0 and placed
    if not placed:
        for k in ('foods', 'heads', 'bodies', 'dones', 'orientations', 'boost_this_step'):
            st[k][...] = 0
        for i in range(N):
            _lay_multi(*_multi_env(st, i), S, rng)
    return st


def _multi_env(st, i):
    """views of env i: food (C), heads (K, C), bodies (K, C), dones (K)"""
    N = st['foods'].shape[0]
    K = st['heads'].shape[0] // N
    return (st['foods'][i].reshape(-1), st['heads'].reshape(N, K, -1)[i], st['bodies'].reshape(N, K, -1)[i],
            st['dones'].reshape(N, K)[i])


# ------------------------------------------------------------------------------------------------ corruptions

def _cell_of(b, v):
    return int(np.nonzero(b == v)[0][0])


def _single_kinds():
    """name -> (function(e (3, C), cell), takes a cell): the variants of tests/golden/make_golden_checker.py"""
    def L(e): return int(e[2].max())
    def head(e): return _cell_of(e[2], L(e))
    def tail(e): return _cell_of(e[2], 1)
    def food(e): return int(np.nonzero(e[0])[0][0])

    def valid(e, c): pass
    def two_heads(e, c): e[1, c] = 1
    def no_head(e, c): e[1] = 0
    def food_value_2(e, c): e[0, food(e)] = 2
    def food_value_2_elsewhere(e, c): e[0, c] = 2
    def no_body(e, c): e[2] = 0
    def no_snake_at_all(e, c): e[1] = 0; e[2] = 0
    def body_value_2_missing(e, c): e[2, _cell_of(e[2], 2)] = 0
    def head_on_the_tail(e, c): t = tail(e); e[1] = 0; e[1, t] = 1
    def length_2_snake(e, c): n, hd = _cell_of(e[2], L(e) - 1), head(e); e[2] = 0; e[2, n] = 1; e[2, hd] = 2
    def food_under_the_head(e, c): e[0] = 0; e[0, head(e)] = 1
    def two_foods(e, c): e[0, c] = 1
    def no_food(e, c): e[0] = 0
    def body_value_2_twice(e, c): e[2, c] = 2
    def values_3_3_sum_is_triangular(e, c): m = _cell_of(e[2], 2); e[2, tail(e)] = 0; e[2, m] = 3
    def head_value_too_large(e, c): e[2, head(e)] = L(e) + 1
    def food_under_the_tail(e, c): e[0] = 0; e[0, tail(e)] = 1
    def stray_larger_body_value(e, c): e[2, c] = L(e) + 1
    added = ('two_heads', 'food_value_2_elsewhere', 'two_foods', 'body_value_2_twice', 'stray_larger_body_value')
    fns = [valid, two_heads, no_head, food_value_2, food_value_2_elsewhere, no_body, no_snake_at_all, body_value_2_missing,
           head_on_the_tail, length_2_snake, food_under_the_head, two_foods, no_food, body_value_2_twice,
           values_3_3_sum_is_triangular, head_value_too_large, food_under_the_tail, stray_larger_body_value]
    return {fn.__name__: (fn, fn.__name__ in added) for fn in fns}


SINGLE_KINDS = _single_kinds()
SINGLE_ACCEPTED = ('valid', 'values_3_3_sum_is_triangular', 'food_under_the_tail')   # the reference accepts these
SINGLE_COVER = ('food_value_2', 'no_snake_at_all', 'head_on_the_tail', 'body_value_2_missing', 'food_under_the_head', 'two_foods')


def _multi_kinds():
    """name -> (function(f, h, b, d, s, o, cell), takes a cell, needs two snakes): s is the snake the corruption aims
    at, o another one.  The generator's variants, and: every snake dead and cleared under a food value of 2 (the food bit
    must stay clear), an overlap of two stray cells, a stray body value, a dead and cleared snake with one cell left"""
    def L(b, s): return int(b[s].max())
    def head(b, s): return _cell_of(b[s], L(b, s))

    def valid(f, h, b, d, s, o, c): pass
    def snake_over_snake(f, h, b, d, s, o, c): b[s] = np.maximum(b[s], b[o])
    def snake_on_top_of_snake(f, h, b, d, s, o, c): b[o] = b[s]; h[o] = h[s]
    def dead_snake_with_a_body(f, h, b, d, s, o, c): d[s] = 1
    def dead_snake_cleared(f, h, b, d, s, o, c): d[s] = 1; h[s] = 0; b[s] = 0
    def two_heads(f, h, b, d, s, o, c): h[s, c] = 1
    def no_head(f, h, b, d, s, o, c): h[s] = 0
    def body_value_2_missing(f, h, b, d, s, o, c): b[s, _cell_of(b[s], 2)] = 0
    def head_on_the_tail(f, h, b, d, s, o, c): t = _cell_of(b[s], 1); h[s] = 0; h[s, t] = 1
    def food_under_the_head(f, h, b, d, s, o, c): f[head(b, s)] = 1
    def food_value_2(f, h, b, d, s, o, c): f[c] = 2
    def living_snake_without_cells(f, h, b, d, s, o, c): h[s] = 0; b[s] = 0
    def all_dead_nothing_cleared(f, h, b, d, s, o, c): d[...] = 1
    def all_dead_all_cleared(f, h, b, d, s, o, c): d[...] = 1; h[...] = 0; b[...] = 0
    def snake_of_length_2(f, h, b, d, s, o, c): n, hd = _cell_of(b[s], L(b, s) - 1), head(b, s); b[s] = 0; b[s, n] = 1; b[s, hd] = 2
    def all_dead_cleared_food_2(f, h, b, d, s, o, c): d[...] = 1; h[...] = 0; b[...] = 0; f[c] = 2
    def overlap_segment(f, h, b, d, s, o, c): b[s, c] = 1; b[o, c] = 2
    def stray_body_value(f, h, b, d, s, o, c): b[s, c] = 2
    def dead_snake_stray_cell(f, h, b, d, s, o, c): d[s] = 1; h[s] = 0; b[s] = 0; b[s, c] = 1
    added = ('two_heads', 'food_value_2', 'all_dead_cleared_food_2', 'overlap_segment', 'stray_body_value', 'dead_snake_stray_cell')
    pair = ('snake_over_snake', 'snake_on_top_of_snake', 'overlap_segment')
    fns = [valid, snake_over_snake, snake_on_top_of_snake, dead_snake_with_a_body, dead_snake_cleared, two_heads, no_head,
           body_value_2_missing, head_on_the_tail, food_under_the_head, food_value_2, living_snake_without_cells,
           all_dead_nothing_cleared, all_dead_all_cleared, snake_of_length_2, all_dead_cleared_food_2, overlap_segment,
           stray_body_value, dead_snake_stray_cell]
    return {fn.__name__: (fn, fn.__name__ in added, fn.__name__ in pair) for fn in fns}


MULTI_KINDS = _multi_kinds()
MULTI_ACCEPTED = ('valid', 'dead_snake_cleared', 'all_dead_all_cleared', 'all_dead_cleared_food_2')
MULTI_COVER = ('food_value_2', 'living_snake_without_cells', 'head_on_the_tail', 'body_value_2_missing', 'food_under_the_head',
               'overlap_segment', 'dead_snake_with_a_body')


def multi_kind_names(K):
    return [k for k, (_, _, pair) in MULTI_KINDS.items() if K > 1 or not pair]


# ------------------------------------------------------------------------------------------------ batches

class Batch(object):
    """state: the corrupted batch ((N, 3, S, S) array, or a MultiSnake state dict); base: the valid batch it was made
    from; kinds / cells / targets: what was done to each env (cell -1: the kind adds no cell)"""

    def __init__(self, base, state, S, K=None, seed=0):
        self.base, self.state, self.S, self.K, self.seed = base, state, S, K, seed
        self.N = (base if K is None else base['foods']).shape[0]
        self.kinds, self.cells, self.targets = ['valid'] * self.N, [-1] * self.N, [0] * self.N


def _copy(state):
    return {k: v.copy() for k, v in state.items()} if isinstance(state, dict) else state.copy()


def _corrupt_single(batch, i, kind, cell, tail=False, rng=None):
    S, C = batch.S, batch.S * batch.S
    fn, takes_cell = SINGLE_KINDS[kind]
    rng = rng or np.random.RandomState(batch.seed * 7919 + i)
    e = batch.state[i].reshape(3, C)
    e[...] = batch.base[i].reshape(3, C)
    if not takes_cell:
        cell = -1
    if tail or (cell >= 0 and e[:, cell].any()):   # the cell has to be free, or the snake in the last group of 64
        _lay_single(e, S, rng, avoid=(cell,) if cell >= 0 else (), tail=tail)
        batch.base[i].reshape(3, C)[...] = e
    before = e.copy()
    fn(e, cell)
    assert kind == 'valid' or not np.array_equal(before, e), (kind, cell)
    batch.kinds[i], batch.cells[i] = kind, cell


def single_tail_room(S):
    """can a snake of three cells and a food lie inside the last group of 64?"""
    return S * S - tail_start(S * S) >= 6


def single_batch(S, N, seed):
    """N envs of S x S, env i with kind (i + seed) mod 18 at the cell the list gives for (i, seed); every other env of
    a kind that does not add a cell has its snake and food inside the last group of 64, where that group has the room.
    Env 0 and env N - 1 take their kinds from SINGLE_COVER, by the seed, so that a few seeds put every bit there"""
    base = _valid_single(S, N, seed)
    batch = Batch(base, base.copy(), S, seed=seed)
    names, cells = list(SINGLE_KINDS), cell_list(S * S)
    for i in range(N):
        kind = names[(i + seed) % len(names)]
        if i == 0:
            kind = SINGLE_COVER[seed % len(SINGLE_COVER)]
        elif i == N - 1:
            kind = SINGLE_COVER[(seed + 3) % len(SINGLE_COVER)]
        cell = cells[(i // len(names) + i + seed) % len(cells)]
        tail = single_tail_room(S) and not SINGLE_KINDS[kind][1] and (i // 2) % 2 == 1
        _corrupt_single(batch, i, kind, cell, tail)
    return batch


def _corrupt_multi(batch, i, kind, cell, s, tail=False, rng=None):
    S, K, C = batch.S, batch.K, batch.S * batch.S
    fn, takes_cell, pair = MULTI_KINDS[kind]
    assert K > 1 or not pair, kind
    rng = rng or np.random.RandomState(batch.seed * 7919 + i)
    o = (K - 1 if s == 0 else 0) if K > 1 else 0
    env, benv = _multi_env(batch.state, i), _multi_env(batch.base, i)
    for a, v in zip(env, benv):
        a[...] = v
    f, h, b, d = env
    if not takes_cell:
        cell = -1
    taken = cell >= 0 and (f[cell] != 0 or h[:, cell].any() or b[:, cell].any())
    needs_snakes = kind not in ('valid', 'all_dead_nothing_cleared', 'all_dead_all_cleared', 'all_dead_cleared_food_2')
    if tail or taken or (needs_snakes and (d[s] or d[o])):  # the cell free, the two snakes alive, or both in the last 64 cells
        _lay_multi(f, h, b, d, S, rng, avoid=(cell,) if cell >= 0 else (), tail=tail)
        for a, v in zip(env, benv):
            v[...] = a
    before = [a.copy() for a in env]
    fn(f, h, b, d, s, o, cell)
    assert kind == 'valid' or any(not np.array_equal(x, y) for x, y in zip(before, env)), (kind, cell)
    batch.kinds[i], batch.cells[i], batch.targets[i] = kind, cell, s


def multi_tail_room(K, S):
    C = S * S
    return C - tail_start(C) >= 12


def multi_batch(K, S, N, seed):
    """N envs of K snakes on S x S, env i with kind (i + seed) mod the number of kinds (two-snake kinds left out at
    K = 1), aimed at snake 0 and snake K - 1 in turn, at the cell the list gives for (i, seed); env 0 and env N - 1 take
    their kinds from MULTI_COVER by the seed"""
    base = _valid_multi(K, S, N, seed)
    batch = Batch(base, _copy(base), S, K=K, seed=seed)
    names, cells = multi_kind_names(K), cell_list(S * S, multi=True)
    cover = [k for k in MULTI_COVER if k in names]
    for i in range(N):
        kind = names[(i + seed) % len(names)]
        if i == 0:
            kind = cover[seed % len(cover)]
        elif i == N - 1:
            kind = cover[(seed + 3) % len(cover)]
        cell = cells[(i // len(names) + i + seed) % len(cells)]
        s = 0 if (i // len(names) + i) % 2 == 0 else K - 1
        tail = multi_tail_room(K, S) and not MULTI_KINDS[kind][1] and (i // 2) % 2 == 1
        _corrupt_multi(batch, i, kind, cell, s, tail)
    return batch


def needle(batch, p, kind, cell):
    """the batch's valid envs, and env p with `kind` at `cell` (snake K - 1 for MultiSnake): one failing env"""
    out = Batch(_copy(batch.base), _copy(batch.base), batch.S, K=batch.K, seed=batch.seed)
    if batch.K is None:
        _corrupt_single(out, p, kind, cell)
    else:
        _corrupt_multi(out, p, kind, cell, batch.K - 1)
    return out


def without_tail(state, K=None):
    """the state with the last group of 64 cells of every plane cleared (coverage: does a bit depend on those cells?)"""
    out = _copy(state)
    for a in ([out] if K is None else [out['foods'], out['heads'], out['bodies']]):
        C = a.shape[-1] * a.shape[-2]
        a.reshape(a.shape[0], -1, C)[:, :, tail_start(C):] = 0
    return out


# ------------------------------------------------------------------------------------------------ the cases of the tests
# (tests/test_checker_batches_gpu.py runs the kernels on them; tests/test_checker_batches_cpu.py proves them first)

# every cells-per-lane tier of check_kernel (2, 4, 8, 16, 24, 32, 48, 64) at both ends; 75 envs: 19 workgroups of four
# waves, 16 of them permuted over the XCDs, three stragglers, an idle wave in the last; and one env on its own
SINGLE_CASES = [(S, 75) for S in (5, 8, 9, 11, 12, 16, 17, 22, 23, 32, 33, 39, 40, 45, 46, 55, 56, 64)] + [(9, 1)]
# a snake as one item of 11 rows of 64 cells (S <= 26), two (S = 27, 36: 11 + 10 rows) and three (S = 46: nine items, the
# odd tail of the double-buffered loop); 64 snakes on the largest grid; 2049 envs: four waves per workgroup and a straggler
MULTI_CASES = [(1, 10, 75), (3, 12, 75), (4, 25, 75), (2, 27, 75), (10, 36, 75), (3, 46, 75), (64, 64, 2), (3, 12, 2049), (2, 27, 2049)]
NEEDLE_SINGLE = [(9, 75), (25, 75)]
NEEDLE_MULTI = [(3, 12, 75), (3, 12, 2049)]
NEEDLE_KINDS_SINGLE = ('two_foods', 'body_value_2_twice')          # second food; stray body value (at cell C - 1)
# MultiSnake has no one-food check (a second food is a valid state): its food needle is a food value of 2
NEEDLE_KINDS_MULTI = ('food_value_2', 'overlap_segment', 'dead_snake_with_a_body', 'stray_body_value')

_cache = {}


def single_case(S, N):
    """the batch of SINGLE_CASES / NEEDLE_SINGLE (built once, shared, never written to: copy before editing)"""
    cases = SINGLE_CASES + [c for c in NEEDLE_SINGLE if c not in SINGLE_CASES]
    if ('s', S, N) not in _cache:
        _cache[('s', S, N)] = single_batch(S, N, cases.index((S, N)))
    return _cache[('s', S, N)]


def multi_case(K, S, N):
    if ('m', K, S, N) not in _cache:
        _cache[('m', K, S, N)] = multi_batch(K, S, N, MULTI_CASES.index((K, S, N)))
    return _cache[('m', K, S, N)]


def needle_positions(N):
    return sorted({p for p in (0, 1, 3, 4, 63, 64, N - 2, N - 1) if 0 <= p < N})


def needles(batch):
    """(p, kind, cell, needle batch) for every position and needle kind; the added cell alternates between C - 1 and
    the rest of the list, the stray body value always sits at C - 1"""
    C = batch.S * batch.S
    cells = cell_list(C, multi=batch.K is not None)
    kinds = NEEDLE_KINDS_SINGLE if batch.K is None else NEEDLE_KINDS_MULTI
    for j, p in enumerate(needle_positions(batch.N)):
        for kind in kinds:
            cell = C - 1 if kind in ('body_value_2_twice', 'stray_body_value') or j % 2 == 0 else cells[j % len(cells)]
            yield p, kind, cell, needle(batch, p, kind, cell)
