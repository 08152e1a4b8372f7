"""CPU: the conditions the cases of tests/float_special_cases.py must meet, on the oracle alone — the case set tells the clamp-first
formula (the defect the float sampler had: the second tap of an axis kept at weight 0 below the first texel centre) from the contract
wherever texels 0 and 1 make them differ, and the two agree for every other position of a special texel, so the defect is confined to the
low clamp.  tests/test_gpu_float_specials.py holds the device to the oracle on the same cases."""
import ctypes
import ctypes.util
import time

import numpy as np
import pytest

import float_special_cases as S

F = np.float32


def test_the_vectorised_fmaf_is_libm_s():
    libm = ctypes.CDLL(ctypes.util.find_library("m"))
    libm.fmaf.restype = ctypes.c_float
    libm.fmaf.argtypes = [ctypes.c_float] * 3
    rng = np.random.default_rng(5)
    n = 60000
    a = rng.normal(size=n).astype(F); b = rng.normal(size=n).astype(F)
    # sums that cancel, sums a half ulp away from a float (the double-rounding cases), huge, tiny and special operands
    c = np.where(rng.uniform(size=n) < 0.5, -(a * b).astype(F), rng.normal(size=n).astype(F)).astype(F)
    a[:2000] = (1 + rng.integers(0, 2 ** 23, 2000) * 2.0 ** -23).astype(F); b[:2000] = (1 + rng.integers(0, 2 ** 23, 2000) * 2.0 ** -23).astype(F)
    c[:2000] = (rng.choice([2.0 ** -24, -2.0 ** -24, 2.0 ** -25, 3 * 2.0 ** -25], 2000)).astype(F)
    edge = np.array([0.0, -0.0, 1.0, 3e38, -3e38, 1e-45, np.inf, -np.inf, np.nan, 0.5, 0.9e37], F)
    ea, eb, ec = [v.reshape(-1) for v in np.meshgrid(edge, edge, edge, indexing="ij")]
    a, b, c = np.concatenate([a, ea]), np.concatenate([b, eb]), np.concatenate([c, ec])
    want = np.array([libm.fmaf(float(x), float(y), float(z)) for x, y, z in zip(a, b, c)], F)
    got = S.fmaf(a, b, c)
    nan = np.isnan(want)
    assert (np.isnan(got) == nan).all()
    assert (got[~nan].view(np.uint32) == want[~nan].view(np.uint32)).all()


def test_the_case_set_is_what_the_module_says():
    cases = S.cases()
    assert len({c.name for c in cases}) == len(cases)
    main = [c for c in cases if c.main]
    for channels in (1, 2):
        for axis in range(3):
            n = S._size(S.MAIN, axis)
            for special in S.SPECIALS:
                got = {(c.index, c.channel) for c in main if c.channels == channels and c.axis == axis and c.special == special}
                assert {i for i, _ in got} == {0, 1, 3, 4, n - 2, n - 1}
                if channels == 2:
                    assert {(1, 0), (1, 1)} <= got and {ch for _, ch in got} == {0, 1}
    assert {c.dims for c in cases} == {S.MAIN} | set(S.SHORT) and all(min(d) <= 2 and 1 in d and 2 in d for d in S.SHORT) and min(S.MAIN) >= 6
    assert sum(c.special == "both" for c in cases) == 1
    for c in cases:
        special = ~(np.abs(c.texels) < 1.0)
        assert special.sum() == (1 if len(S.SPECIALS.get(c.special, (0, 0))) == 1 else 2)
        finite = c.texels[~special]
        assert finite.min() >= F(0.2) and finite.max() <= F(0.9)
        assert c.atlas == bool((np.abs(c.texels) < 1e37).all())
        assert (2000 if c.main else 1000) <= len(c.points) <= 4000     # (the walk of a one-texel axis has 15 values)
        walk = c.points[:, c.axis]
        n = S._size(c.dims, c.axis)
        for v in [-np.inf, np.inf, 0.0, 1.0, F(0.5) / F(n)] + [F((k + 0.5) / n) for k in range(n)] + [F(k / n) for k in range(1, n)]:
            assert (walk == F(v)).any(), (c, v)
        assert np.isnan(walk).any()
        # entry 0 of the transfer function is what no finite sample of the noise reaches
        assert (c.tf[:, 0] == 255).all() and (c.tf[c.channels - 1:, 1:] <= 200).all() and (c.channels == 1 or (c.tf[0] == 255).all())


def test_the_cases_separate_the_clamp_first_formula_from_the_oracle_at_texel_1_and_only_there(oracle):
    """for every axis, special value and both float formats the cases the module marks `differs` (index 1; the overflowing pair on texels 0
    and 1) hold at least 50 points where the oracle and the clamp-first statement give different colours, under both filters that blend; for
    every other index (0, 3, 4, N - 2, N - 1) and the pair below the atlas threshold the two agree at EVERY point, bit for bit; and all of it
    is generated in under 10 s"""
    t0 = time.perf_counter()
    seen = set()
    for c in S.cases():
        for filt in ("linear", "quasicubic"):
            want = S.expected(oracle, c, filt)
            wrong = S.clamp_first(oracle, c, filt)
            assert not np.isnan(want).any() and not np.isnan(wrong).any()          # the transfer function's texels are finite
            differ = (want.view(np.uint32) != wrong.view(np.uint32)).any(axis=1)
            if c.differs:
                assert differ.sum() >= 50, (c, filt, int(differ.sum()))
                # ... all of them below the first texel centre of the axis under test (or at a NaN coordinate), where the poisoned sample shows entry 0
                u = c.points[differ, c.axis].astype(np.float64) * S._size(c.dims, c.axis) - 0.5
                assert (~(u >= 0)).all(), (c, filt)
                assert (wrong[differ] == 1.0).all(), (c, filt)
                if c.main:
                    seen.add((c.channels, c.axis, c.special))
            else:
                assert not differ.any(), (c, filt, int(differ.sum()), c.points[differ][:3])
        S.expected(oracle, c, "nearest")
    assert seen == {(ch, a, s) for ch in (1, 2) for a in range(3) for s in ("nan", "+inf", "-inf", "overflow")}
    assert time.perf_counter() - t0 < 10.0


def test_the_batch_probe_is_the_single_probe(oracle):
    c = next(c for c in S.cases() if c.name == "rg32f-9x6x7-x-ch1-nan-1")
    L = oracle.lib()
    buf = np.empty(4, F)
    for filt in S.FILTERS:
        sc = oracle.OracleScene(c.texels, filt, tf=c.tf)
        want = S.expected(oracle, c, filt)
        for k in range(0, len(c.points), 7):
            L.vpo_sample_volume_color(ctypes.byref(sc.c), *[float(v) for v in c.points[k]], buf.ctypes.data_as(ctypes.c_void_p))
            assert buf.tobytes() == want[k].tobytes()
