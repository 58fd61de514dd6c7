"""GPU parity: the one-pass per-variable kernel at 33 - 64 particles (``lhvi_pbp_var_fused64``: one variable per wavefront)
against the three kernels it stands for -- every array of the state after whole sweeps, bit for bit."""
import numpy as np
import pytest

from test_gpu_pbp import _init, paper_popularity

pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module')
def api():
    from lhvi import _abi
    _abi.require_gpu()
    return _abi


def _narrowed(flat, half=1.5):
    """the continuous domain of a flat graph cut to [-half, half], bounds and integral points together: proposals as wide as the
    domain, so that many draws are clipped to a bound (exact duplicates)"""
    for d in np.flatnonzero(flat.dom_cont.astype(bool)):
        lo, hi = int(flat.dom_ptr[d]), int(flat.dom_ptr[d + 1])
        flat.dom_lo[d], flat.dom_hi[d] = -half, half
        flat.dom_val[lo:hi] = np.linspace(-half, half, hi - lo)
    return flat


# case -> (n, rule, T, graph)
CASES = {
    'n64': (64, 'simple', 32, 'mrf'),
    'n33': (33, 'simple', 32, 'mrf'),                  # lanes beyond np idle
    'n48': (48, 'simple', 32, 'mrf'),
    'n64 T48': (64, 'simple', 48, 'mrf'),              # two integral points per lane over 32 lanes
    'n64 EP': (64, 'EP', 32, 'mrf'),
    'n40 EP T64': (40, 'EP', 64, 'mrf'),
    'n64 deg12': (64, 'simple', 32, 'mrf deg12'),      # a row spans several chunks and several proposal passes
    'n64 narrow': (64, 'simple', 32, 'mrf narrow'),    # clipped draws: duplicate particles
    'n48 EP narrow': (48, 'EP', 32, 'mrf narrow'),
    'hlbp n40': (40, 'simple', 32, 'hlbp'),            # lifted, with edge counts
    'hmln hubs n64': (64, 'simple', 32, 'hmln'),       # hub rows stay with the three kernels
}


@pytest.mark.parametrize('case', list(CASES))
def test_fused64_kernel_equals_the_three_kernels(api, case):
    """``fused_max_particles = 64`` (the new class: hidden continuous variables with 32 < n <= 64, degree <= prop_slice, T <= 64, served
    by ``pbp_var_fused_kernel<64, 16 | 32>``) against ``= 32`` (``lhvi_pbp_v2f`` + ``lhvi_pbp_proposal`` +
    ``lhvi_pbp_resample_uniq``): five sweeps and a last one, then ``torch.equal`` on every array of the state"""
    import torch
    from lhvi import synth
    from lhvi.pbp import EPBP, HybridLBP
    n, approx, T, graph = CASES[case]
    runs = []
    for fused_max in (64, 32):
        if graph == 'hlbp':
            g, table = paper_popularity(30, 4, seed=9)
            bp = HybridLBP(g, n=n, proposal_approximation=approx, sampler='device', seed=4)
            bp.fused_var_kernel, bp.fused_max_particles = True, fused_max
            bp.run(6)
        else:
            if graph == 'hmln':
                flat, keys = synth.paper_popularity_flat(150, 4, seed=2)          # topics touch > 64 factors: not fused
            else:
                flat = synth.hybrid_mrf_flat(V=3000, deg=12 if 'deg12' in graph else 4, seed=37, frac_discrete=0.3, T=T)
                if 'narrow' in graph:
                    flat = _narrowed(flat)
            bp = EPBP(None, n=n, proposal_approximation=approx, sampler='device', seed=6)
            bp.fused_var_kernel, bp.fused_max_particles = True, fused_max
            bp._setup(None, flat=flat)
            _init(api, bp)
            for _ in range(5):
                bp.sweep(last=False)
            bp.sweep(last=True)
        torch.cuda.synchronize()
        runs.append(bp)
    a, b = runs
    # the new class is there in the first state and absent in the second (which has nothing to fuse at this n)
    assert a._fused is not None and sum(a._fused['counts']) == 0 and sum(a._fused['counts64']) > 0 and a._fused['desc64'] is not None
    assert b._fused is None
    c64a, c64b = a._fused['counts64']
    if graph.startswith('mrf'):
        assert (c64a > 0) == (T <= 32) and (c64b > 0) == (T > 32)
        fl = a.flat
        assert c64a + c64b == int((fl.var_hidden & fl.var_cont).sum())             # every hidden continuous variable is in the class
    if graph == 'hmln':
        assert a._fused['n_prop_rest'] > 0 and a.n_prop_hub > 0                    # the hub rows stay with the three kernels
    for name in ('q_dev', 'eta', 'particles', 'old_particles', 'uniq', 'v2f', 'f2v'):
        assert torch.equal(getattr(a, name), getattr(b, name)), name
    assert bool(torch.isfinite(a.q_dev[torch.from_numpy(a.flat.var_hidden & a.flat.var_cont).to(a.q_dev.device)]).all())
    if 'narrow' in graph:
        # duplicate particles among the live lanes of the new class's variables, and the mask is the exact first-occurrence mask
        fl = a.flat
        vs = np.flatnonzero(fl.var_hidden & fl.var_cont)
        P, U = a.particles.cpu().numpy()[vs, :n], a.uniq.cpu().numpy()[vs, :n].astype(bool)
        assert int((~U).sum()) > 100
        first = np.array([[P[i, j] not in P[i, :j] for j in range(n)] for i in range(min(300, vs.size))])
        np.testing.assert_array_equal(U[:first.shape[0]], first)
