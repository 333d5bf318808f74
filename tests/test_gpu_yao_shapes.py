"""gc_yao_* where tests/test_gpu_yao.py does not go: batches whose layout tile holds 2, 4 and 8 instances (512 to 2 051
sessions, the runs of q sessions of the M1 kernels below, at and above their session tile), every session tile (4 to 64) and
pieces of 64 and 80 bytes, message tails of 0 to 3 words and labels across piece boundaries by 4, 8 and 12 bytes, the largest
LDS shapes create accepts, the shapes it refuses, and directed results for the decode kernels.  Every case is one whole run
(send, OT in the clear, accept, eval, both results) and EVERY session of it is compared byte for byte with the Python
restatement through tests/yao_cases.py; tests/test_yao_shape_cases_host.py asserts that the inputs hit these edges."""
import numpy as np
import pytest

from mpc_amd import engine
from tests import py_yao_reference as ref
from tests import yao_cases as cases
from tests import yao_shape_cases as sc

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx():
    c = engine.Context(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def device_circuit(ctx):
    """name -> the DeviceCircuit of sc.circuit(name), made once"""
    made = {}

    def get(name):
        if name not in made:
            made[name] = engine.DeviceCircuit(ctx, sc.circuit(name)[0])
        return made[name]

    yield get
    for dc in made.values():
        dc.close()


def set_shape(monkeypatch, tile, piece):
    """GC_YAO_TILE / GC_YAO_PIECE as create will read them (None: the default)"""
    for name, v, default in (("GC_YAO_TILE", tile, sc.DEFAULT_SHAPE[0]), ("GC_YAO_PIECE", piece, sc.DEFAULT_SHAPE[1])):
        if v is None:
            monkeypatch.delenv(name, raising=False)
        else:
            monkeypatch.setenv(name, str(v))
    want = (tile or sc.DEFAULT_SHAPE[0], piece or sc.DEFAULT_SHAPE[1])
    assert engine.yao_kernel_shape() == want
    return want


def compare(got, name, keylen, sessions, want_of):
    S = len(sessions)
    assert got["m1"].shape[0] == S
    keys = cases.rows_of(sessions, "key")
    assert (got["m1"][:, 4:4 + keylen] == keys).all(), "M1 of sessions %s carries another session's key" % \
        np.flatnonzero((got["m1"][:, 4:4 + keylen] != keys).any(1))[:8]
    for s in range(S):
        cases.assert_equal_to_reference(got, want_of(s), s)


def run_and_compare(device_circuit, name, keylen, S, path=0, instances=None):
    """one whole DeviceYao.run of sessions 0 .. S of circuit `name`; every session against its reference"""
    g = sc.geometry(name, keylen)
    sessions = sc.sessions(name, keylen, S)
    dy = cases.DeviceYao(device_circuit(name), g, S)
    try:
        if instances is not None:
            assert dy.gb.batch.tile_instances == dy.ev.batch.tile_instances == instances
        if path:
            dy.gb.batch.set_keyed_path(path)
            dy.ev.batch.set_keyed_path(path)
            assert dy.gb.batch.keyed_path == dy.ev.batch.keyed_path == path
        got = dy.run(sessions)
    finally:
        dy.close()
    compare(got, name, keylen, sessions, lambda s: sc.reference(name, keylen, s))
    return got


# ---- a. tiled batch layouts at the default M1 geometry -----------------------------------------------------------------------

@pytest.mark.parametrize("S,instances", [(511, 1), (512, 2), (513, 2), (1024, 4), (1027, 4), (2048, 8), (2051, 8)])
def test_tiled_batch_layouts(device_circuit, monkeypatch, S, instances):
    """layout tiles of 1, 2, 4 and 8 instances against the session tile of 4: runs of q = 1, 2 and 4 sessions, the layout tile
    above the session tile, and a ragged last layout tile in each"""
    set_shape(monkeypatch, None, None)
    run_and_compare(device_circuit, "small", 32, S, instances=instances)


def test_tiled_layout_on_keyed_path_2_gives_the_same_bytes(device_circuit, monkeypatch):
    set_shape(monkeypatch, None, None)
    one = run_and_compare(device_circuit, "small", 32, 1027, instances=4)
    two = run_and_compare(device_circuit, "small", 32, 1027, path=2, instances=4)
    for k in ("m1", "m2", "m3", "len3", "bits", "ebits"):
        assert (one[k] == two[k]).all(), k


# ---- b. session tile against layout tile, pieces of 64 bytes ----------------------------------------------------------------

@pytest.mark.parametrize("tile,S,instances", [(8, 1027, 4), (64, 513, 2), (16, 2051, 8)])
def test_session_tile_against_layout_tile(device_circuit, monkeypatch, tile, S, instances):
    """(8, 1 027): q = 4 below the tile of 8, two runs a workgroup and a ragged last one; (64, 513): 32 runs of 2; (16,
    2 051): the layout tile of 8 below the session tile"""
    set_shape(monkeypatch, tile, 64)
    run_and_compare(device_circuit, "small", 32, S, instances=instances)


# ---- c. every template instance and the small pieces ------------------------------------------------------------------------

@pytest.mark.parametrize("piece", [64, 80])
@pytest.mark.parametrize("tile", [4, 8, 16, 32, 64])
def test_every_session_tile_at_small_pieces(device_circuit, monkeypatch, tile, piece):
    set_shape(monkeypatch, tile, piece)
    for S in (tile - 1, 2 * tile + 1):
        run_and_compare(device_circuit, "small", 32, S, instances=1)


@pytest.mark.parametrize("keylen", [16, 24])
def test_short_keys_at_pieces_of_64(device_circuit, monkeypatch, keylen):
    """keylen 24: no tail words and a last piece that is exactly full"""
    set_shape(monkeypatch, 4, 64)
    for S in (3, 9):
        run_and_compare(device_circuit, "small", keylen, S)


# ---- d. tails of 1 and 3 words, labels across a boundary by 4 and 12 bytes --------------------------------------------------

@pytest.mark.parametrize("piece", [64, None])
@pytest.mark.parametrize("keylen", [16, 24])
@pytest.mark.parametrize("bits", [67, 69])
def test_tails_and_label_crossings(device_circuit, monkeypatch, bits, keylen, piece):
    set_shape(monkeypatch, 4, piece)
    run_and_compare(device_circuit, "and%d" % bits, keylen, 5)


# ---- e. the largest LDS shapes -----------------------------------------------------------------------------------------------

@pytest.mark.parametrize("tile,piece,S", [(32, 4096, 33), (8, 16384, 9)])
def test_the_largest_lds_shapes(device_circuit, monkeypatch, tile, piece, S):
    """about 131 KB of LDS a workgroup, on the circuit whose M1 is five pieces of 4 096 and two of 16 384"""
    set_shape(monkeypatch, tile, piece)
    run_and_compare(device_circuit, "wide", 32, S)


# ---- f. what create refuses --------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("tile,piece", [(64, 4096), (5, 4096), (4, 48), (4, 72), (4, 16400)])
def test_create_refuses_a_bad_kernel_shape(device_circuit, monkeypatch, tile, piece):
    """(64, 4096): LDS past 160 KiB"""
    monkeypatch.setenv("GC_YAO_TILE", str(tile))
    monkeypatch.setenv("GC_YAO_PIECE", str(piece))
    dc = device_circuit("small")
    with pytest.raises(engine.EngineError) as e:
        engine.yao_kernel_shape()
    assert e.value.code == engine.GC_E_ARG and b"GC_YAO_TILE" in engine.lib().gc_last_error()
    for handle in (engine.YaoGarbler, engine.YaoEvaluator):
        with pytest.raises(engine.EngineError) as e:
            handle(dc, 3, 9, 32, 3)
        assert e.value.code == engine.GC_E_ARG and b"GC_YAO_TILE" in engine.lib().gc_last_error()
    monkeypatch.delenv("GC_YAO_TILE")
    monkeypatch.delenv("GC_YAO_PIECE")
    assert engine.yao_kernel_shape() == sc.DEFAULT_SHAPE
    run_and_compare(device_circuit, "small", 32, 3)


# ---- g. directed results -----------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("nout", sc.DIRECTED_NOUT)
def test_directed_results_of_the_decode_kernels(device_circuit, monkeypatch, nout):
    """an AND of nout bits with the garbler's bits all one: the result is the evaluator's input.  Zero, the highest bit at 0,
    7, 8, 63, 64 and nout - 1, all ones — one session each in one call, the last decode block with a dead wave"""
    set_shape(monkeypatch, None, None)
    name, vs, sessions = "and%d" % nout, sc.directed_values(nout), sc.directed_sessions(nout)
    g, circ = sc.geometry(name, 32), sc.circuit(name)[0]
    S = len(vs)
    assert S % 4 and S % 16
    dy = cases.DeviceYao(device_circuit(name), g, S)
    try:
        got = dy.run(sessions)
    finally:
        dy.close()
    wants = [cases.reference(circ, g, ses) for ses in sessions]
    for s, v in enumerate(vs):
        direct = sc.directed_expectation(nout, v)
        assert (wants[s]["m3"], wants[s]["len3"], wants[s]["bits"]) == (direct["m3"], direct["len3"], direct["bits"]), hex(v)
        assert int(got["len3"][s]) == direct["len3"], (hex(v), got["len3"][s])
        assert got["m3"][s, :direct["len3"]].tobytes() == direct["m3"], hex(v)
        assert got["bits"][s].tobytes() == direct["bits"] == got["ebits"][s].tobytes(), hex(v)
    compare(got, name, 32, sessions, lambda s: wants[s])
