"""The conditions on the inputs of test_match_capacity_gpu.py (match_inputs.named_cases), at the oracle alone: every named block count
is hit exactly, with the keyframes, the success and the association path the case intends, and the residual blocks at the seam are
loud enough for a comparison at 1e-9 to see any one of them go missing. A target the generator cannot reach fails here."""
import pytest

import match_caps
import match_inputs as mi

CASES = mi.named_cases(match_caps.INSTANTIATIONS)


def test_capacity_table():
    assert match_caps.INSTANTIATIONS["pipeline"][0] == match_caps.TABLE["pipeline"][0] == {2: 622, 1: 710, 0: 995}
    for inst in match_caps.TABLE:
        assert match_caps.INSTANTIATIONS[inst] == match_caps.TABLE[inst], inst
    assert sum(c % 2 for caps, _ in match_caps.TABLE.values() for c in caps.values()) == 3  # three of the twelve are odd
    assert len({c.name for c in CASES}) == len(CASES)


@pytest.mark.parametrize("route", sorted(mi.ROUTES))
def test_every_named_block_count_is_hit(oracle, route):
    quiet, vacuous, n = [], 0, 0
    for c in [c for c in CASES if c.route == route]:
        case = c.steer()
        S = case.ref[-1][1]
        n += 1
        assert S.success == 1 and S.usable == 1, c.name
        assert case.keyframes == c.submap and len(case.sweeps) == c.submap + 1 <= 12, c.name
        assert all(r[2] == min(t + 1, c.submap) for t, r in enumerate(case.ref)), c.name  # every sweep became a keyframe
        assert int(S.num_residual_blocks) == c.target == case.blocks, (c.name, int(S.num_residual_blocks))
        assert int(S.num_residuals) == c.target * (1 if c.cost == 1 else 2), c.name
        assert (c.family == "B" and c.target <= c.cap) or c.target - c.cap in (-1, 0, 1, 2, 256, 257, 512, 513), c.name
        if not c.polar:
            assert max(len(s) for s in case.sweeps) <= 8000, c.name
        path = c.want_path(case.cells)
        if c.pad:
            assert path == 2 and case.cells > 256, (c.name, case.cells)
        elif c.family == "A" and c.route in ("step4", "call") and c.cost != 0:
            assert path == 1, (c.name, case.cells)  # 256 cells reach these counts: the block path
        loud, share = mi.seam_is_loud(case, c.cap)
        if loud is None:
            vacuous += 1
        elif not loud:
            quiet.append((c.name, share))
        if c.route == "call":  # the per-call problem built from the fuser's run has the fuser's count
            clouds, poses = mi.call_inputs(case)
            p = oracle.default_params(**case.kw)
            ret, P, cov, S2 = oracle.register([oracle.Scan(x, p) for x in clouds], poses, p)
            assert ret == 1 and int(S2.num_residual_blocks) == c.target, (c.name, int(S2.num_residual_blocks))
    assert not quiet, quiet
    print("[inputs] %s: %d cases, seam weights restated for %d" % (route, n, n - vacuous))
    assert vacuous <= n // 4, (vacuous, n)  # the restatement of the last build reproduces the fuser's count nearly always
