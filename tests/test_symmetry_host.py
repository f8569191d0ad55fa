"""Board symmetries without a device (include/mssym.h): the ctypes table against the header, the
host cell map against the numpy restatement of tests/symmetry_ref.py and its group properties,
the argument checks, and the imitation config keys. No device needed."""
from __future__ import annotations

import ctypes
import os

import numpy as np
import pytest

import symmetry_ref as R
from conftest import PKG_DIR, ROOT
from test_abi_signatures import parse_headers, table_errors

SYM_H = os.path.join(ROOT, "include", "mssym.h")
NAMES = ["ms_sym_cell_map_host", "ms_sym_expand", "ms_sym_gather", "ms_sym_mean"]


def test_table_matches_the_header():
    from ms_amd import _lib as L
    lib = L.load()
    protos, structs, defines, diag_only = parse_headers([SYM_H])
    table = L.SIGNATURES_SYM
    assert sorted(protos) == NAMES and not structs and not defines and not diag_only
    assert table_errors(table, L._RESTYPES, protos) == []
    others = (L.SIGNATURES, L.SIGNATURES_GROUPED, L.SIGNATURES_EXPERT, L.SIGNATURES_BC)
    assert not any(set(table) & set(t) for t in others)
    with open(os.path.join(PKG_DIR, "libmsenv_diag.so"), "rb") as f:
        diag_image = f.read()
    for name, argtypes in table.items():
        fn = getattr(lib, name)  # the product library exports and binds it
        assert list(fn.argtypes) == argtypes and fn.restype is ctypes.c_int, name
        assert b"\0" + name.encode() + b"\0" in diag_image, f"libmsenv_diag.so lacks {name}"
    # a wrong table is reported: n narrowed to 32 bits, and a parameter dropped
    narrowed = list(table["ms_sym_gather"])
    narrowed[2] = ctypes.c_int32
    errs = table_errors(dict(table, ms_sym_gather=narrowed), L._RESTYPES, protos)
    assert errs and "int64_t n" in errs[0]
    assert table_errors(dict(table, ms_sym_mean=table["ms_sym_mean"][:-1]), L._RESTYPES, protos)
    assert L.ABI_VERSION == 3 and lib.ms_abi_version() == 3
    assert [k for k, _, _ in L.SYM_PLANES] == ["codes", "mask", "best", "labels", "kind"]


@pytest.mark.parametrize("shape", R.SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_cell_map_is_the_numpy_transform_and_a_group(shape):
    from ms_amd.symmetry import cell_map, group_size, inverse
    H, W = shape
    A, G = H * W, group_size(H, W)
    assert G == R.group_size(H, W) == (8 if H == W else 4)
    maps = [cell_map(H, W, g) for g in range(G)]
    X = np.random.default_rng(H * 100 + W).integers(0, 1 << 30, size=(H, W))
    ident = np.arange(A)
    for g, m in enumerate(maps):
        assert m.dtype == np.int32 and m.shape == (A,)
        assert np.array_equal(m, R.cell_map(H, W, g)), g
        assert np.array_equal(X.reshape(-1)[m], np.ascontiguousarray(R.transform(X, g)).reshape(-1)), g
        assert np.array_equal(np.sort(m), ident), f"g {g}: not a permutation"
        assert inverse(g) == R.inverse(g) and inverse(inverse(g)) == g
        assert inverse(g) == (g if g < 4 else {4: 4, 5: 6, 6: 5, 7: 7}[g])
        # out = in[map(g)], then [map(inverse g)]: in[map(g)[map(inv)]] must be in
        assert np.array_equal(m[maps[inverse(g)]], ident), g
    assert np.array_equal(maps[0], ident)
    # closed under composition: applying g then h is some element of the group
    have = {m.tobytes() for m in maps}
    for mg in maps:
        for mh in maps:
            assert mg[mh].tobytes() in have


def test_bad_arguments_are_refused():
    from ms_amd import _lib as L
    from ms_amd.symmetry import cell_map, inverse
    lib = L.load()
    buf = np.full(520, -7, dtype=np.int32)
    host = lambda H, W, g: lib.ms_sym_cell_map_host(H, W, g, buf.ctypes.data)  # noqa: E731
    for g in (4, 5, 6, 7):
        assert host(5, 7, g) == 1
        assert b"ms_sym_cell_map_host" in lib.ms_last_error()
    assert host(5, 7, 3) == 0 and host(4, 4, 7) == 0
    buf[:] = -7
    for H, W, g in ((4, 4, 8), (4, 4, -1), (4, 4, 256), (0, 4, 0), (4, 0, 0), (-1, -1, 0), (513, 1, 0), (1, 513, 0),
                    (27, 19, 0), (1 << 16, 1 << 16, 0)):
        assert host(H, W, g) == 1, (H, W, g)
    assert b"512" in lib.ms_last_error()
    assert (buf == -7).all()  # a refused call writes nothing
    assert lib.ms_sym_cell_map_host(4, 4, 0, None) == 1
    with pytest.raises(L.MsEnvError):
        cell_map(5, 7, 4)
    with pytest.raises(L.MsEnvError):
        cell_map(0, 4, 0)
    with pytest.raises(ValueError):
        inverse(8)
    # the device entry points check before any device work: the pointers are never dereferenced
    fake = ctypes.c_void_p(4096)
    planes = [None] * 11
    gather = lambda rows, g, n, H, W, B: lib.ms_sym_gather(rows, g, n, H, W, B, *planes, None)  # noqa: E731
    assert gather(fake, fake, 0, 4, 4, 4) == 1 and gather(fake, fake, 1 << 31, 4, 4, 4) == 1
    assert gather(fake, None, 4, 4, 4, 4) == 1 and gather(fake, fake, 4, 4, 4, 0) == 1
    assert gather(fake, fake, 4, 0, 4, 4) == 1 and gather(fake, fake, 4, 27, 19, 4) == 1
    assert gather(None, fake, 3, 4, 4, 4) == 1  # identity rows need n == B_src
    assert b"ms_sym_gather" in lib.ms_last_error()
    for fn, who in ((lib.ms_sym_expand, b"ms_sym_expand"), (lib.ms_sym_mean, b"ms_sym_mean")):
        assert fn(fake, 4, 5, 7, 8, fake, None) == 1  # G = 8 on a board that is not square
        assert who in lib.ms_last_error() and b"square" in lib.ms_last_error()
        for G in (0, 2, 3, 16):
            assert fn(fake, 4, 4, 4, G, fake, None) == 1
        assert fn(fake, 0, 4, 4, 4, fake, None) == 1 and fn(fake, 4, 4, 4, 4, None, None) == 1
        assert fn(None, 4, 4, 4, 4, fake, None) == 1 and fn(fake, 4, 32, 32, 4, fake, None) == 1


def test_imitation_config_keys():
    from ms_amd.imitate import BCConfig, imitation_params
    from ms_amd.train import load_config
    assert BCConfig().augment is False and imitation_params({})["augment"] is False
    assert imitation_params({"imitation": {"augment": True, "epochs": 3}})["augment"] is True
    with pytest.raises(ValueError, match="unknown"):
        imitation_params({"imitation": {"augmnet": True}})
    base = load_config(os.path.join(ROOT, "configs", "imitation", "16x16x40_medium.yaml"))
    sym = load_config(os.path.join(ROOT, "configs", "imitation", "16x16x40_medium_sym.yaml"))
    assert sym[1] == base[1] and sym[2] == base[2] and vars(sym[0]) == vars(base[0])
    il0, il1 = imitation_params(base[3]), imitation_params(sym[3])
    assert il1["augment"] is True and il0["augment"] is False and il1["epochs"] >= 1
    assert {k: v for k, v in il1.items() if k not in ("augment", "epochs")} == \
        {k: v for k, v in il0.items() if k not in ("augment", "epochs")}
    assert {k: v for k, v in sym[3].items() if k != "imitation"} == {k: v for k, v in base[3].items() if k != "imitation"}
