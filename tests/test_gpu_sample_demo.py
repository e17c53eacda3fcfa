"""demos/posterior_band.py in-process: the bands it reports are bands (simultaneous at least as wide as pointwise, coverages in [0, 1])."""
import os
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize('gaps', [False, True])
def test_posterior_band_demo(gaps, capsys):
    sys.path.insert(0, os.path.join(ROOT, 'demos'))
    import posterior_band
    out = posterior_band.main(['--T', '600', '--samples', '256'] + (['--gaps'] if gaps else []))
    print(capsys.readouterr().out)
    pw, sim = out['pointwise'], out['simultaneous']
    assert sim['k'] >= pw['k'] > 0
    assert (sim['hi'] - sim['lo'] >= pw['hi'] - pw['lo'] - 1e-12).all()
    assert np.isfinite(sim['lo']).all() and np.isfinite(sim['hi']).all()
    for band in (pw, sim):
        assert 0.0 <= band['coverage'] <= 1.0
    assert sim['coverage'] >= pw['coverage']
    if gaps:
        assert 0.0 <= sim['tail_coverage'] <= 1.0
        assert sim['tail_width'][1] > sim['tail_width'][0]           # the forecast band opens with the horizon
