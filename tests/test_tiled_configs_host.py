"""CPU: the case table of the tiled fp32 conv kernel (tests/tiled_cases.py, run against the fp64 oracle by
tests/test_tiled_configs_gpu.py) is current and complete.  Host-only queries, no GPU: bts_conv3d_kernel, bts_conv3d_fwd_workspace,
bts_conv3d_bwd_data_workspace, bts_conv3d_fwd_can_fuse.

  * every row, under its own switches, is named the symbol it claims, and asks for a workspace exactly where it says the contraction is
    split -- a stale row fails here before any GPU time is spent;
  * every (direction, kind, config) the CLI-default model reaches on the tiled kernel, over the three BASELINE grids of
    test_host_planning.py with default switches, has a row -- a change of thresholds that sends a layer to an untested config fails here;
  * the same with BTS_WINO=0 for the 3x3x3 stride-1 layers, which then all run the tiled kernel: plain, with the fused shortcut output
    (forward) and as the data-gradient pair."""
import pytest

import tiled_cases as T
from test_host_planning import GRIDS, layer_shapes

KIND = {T.K1: 'K1', T.K3S1: 'K3S1', T.K3S2: 'K3S2', T.K3S2T: 'K3S2T'}
FORM = {0: 'plain', T.Y2: 'fused shortcut output', T.X2: 'data-gradient pair'}


@pytest.fixture(scope='module')
def L():
    import bts_amd  # noqa: F401
    from bts_amd._lib import lib
    return lib()


def switches(monkeypatch, env):
    for k in T.SWITCHES:
        monkeypatch.delenv(k, raising=False)
    for k, v in env.items():
        monkeypatch.setenv(k, v)


def describe(key):
    direction, kind, second, sym = key
    return '%s %s %s -> %s' % ('forward' if direction == T.FWD else 'data gradient', KIND[kind], FORM[second],
                               'BTS_ERR_UNSUPPORTED' if sym == T.UNSUPPORTED else 'symbol %d' % sym)


def query(L, direction, kind, n, d, h, w, ci, co, second=0):
    """bts_conv3d_kernel for a layer's call: dense, aligned operands; the workspace the engine's callers pass (none to the fused pair)"""
    return L._bts_conv3d_kernel(direction, kind, n, d, h, w, ci, ci, co, co, 0, second, co if second else 0, 0, 15, 0 if second == T.Y2 else -1)


def uncovered(reached):
    have = {T.key(r) for r in T.ROWS}
    return sorted(describe(k) + ', e.g. %r' % (reached[k],) for k in reached if k not in have)


def test_row_names_are_unique_and_rows_claim_tiled_symbols():
    assert len(T.by_name()) == len(T.ROWS)
    for r in T.ROWS:
        assert r.sym in T.TILED or (r.sym == T.UNSUPPORTED and r.second == T.Y2), r.name
        assert (r.sym >= 8) == (r.kind == T.K1) or r.sym < 0, r.name
        assert not r.second or r.kind == T.K3S1, r.name
        assert (r.second == T.Y2) <= (r.direction == T.FWD) and (r.second == T.X2) <= (r.direction == T.BWD), r.name


@pytest.mark.parametrize('name', [r.name for r in T.ROWS])
def test_row_is_named_the_symbol_it_claims(L, monkeypatch, name):
    r = T.by_name()[name]
    switches(monkeypatch, r.env)
    assert T.named(L, r) == r.sym, (r.name, T.named(L, r))
    need = T.workspace(L, r)
    assert (need > 0) == r.splitk, (r.name, need)
    d, h, w = r.dims
    if r.second == T.Y2:
        assert L._bts_conv3d_fwd_can_fuse(r.n, d, h, w, r.cin, r.cout) == (r.sym != T.UNSUPPORTED), r.name
    if r.second == T.X2:      # bts_conv3d_bwd_data_pair makes one engine call of the pair only where the 3x3x3 gradient asks for no workspace
        assert need == 0 and r.cout % 8 == 0 and r.cin > 4, r.name


def test_every_tiled_config_the_model_reaches_has_a_row(L, monkeypatch):
    switches(monkeypatch, {})
    reached = {}
    for grid in GRIDS:
        for (kind, n, d, h, w, ci, co) in layer_shapes(*grid):
            for direction in (T.FWD, T.BWD):
                sym = query(L, direction, kind, n, d, h, w, ci, co)
                if sym in T.TILED:
                    reached.setdefault((direction, kind, 0, sym), (n, d, h, w, ci, co))
    assert len(reached) >= 10, sorted(reached)      # (the walk found the model's tiled layers at all)
    missing = uncovered(reached)
    assert not missing, 'no row of tests/tiled_cases.py for: ' + '; '.join(missing)


def test_every_tiled_config_behind_the_winograd_forms_has_a_row(L, monkeypatch):
    switches(monkeypatch, T.NOWINO)
    reached = {}
    for grid in GRIDS:
        for (kind, n, d, h, w, ci, co) in layer_shapes(*grid):
            if kind != T.K3S1:
                continue
            shape = (n, d, h, w, ci, co)
            for direction in (T.FWD, T.BWD):
                sym = query(L, direction, kind, *shape)
                if sym in T.TILED:
                    reached.setdefault((direction, kind, 0, sym), shape)
            sym = query(L, T.FWD, kind, *shape, second=T.Y2)
            assert (sym == T.UNSUPPORTED) == (L._bts_conv3d_fwd_can_fuse(*shape) == 0), shape
            if sym in T.TILED or sym == T.UNSUPPORTED:
                reached.setdefault((T.FWD, kind, T.Y2, sym), shape)
            # the pair is one engine call where the 3x3x3 gradient asks for no workspace, dy2 has whole 8-channel groups and Cin > 4
            if L._bts_conv3d_bwd_data_workspace(kind, *shape) == 0 and co % 8 == 0 and ci > 4:
                sym = query(L, T.BWD, kind, *shape, second=T.X2)
                if sym in T.TILED:
                    reached.setdefault((T.BWD, kind, T.X2, sym), shape)
    assert {k[2] for k in reached} == {0, T.Y2, T.X2}, sorted(reached)
    missing = uncovered(reached)
    assert not missing, 'no row of tests/tiled_cases.py for: ' + '; '.join(missing)
