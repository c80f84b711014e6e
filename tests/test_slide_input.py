"""The slide input stage's keywords (``biscuit_amd/slide_input.py``), on the CPU with no engine: ``Heatmap.from_slide`` and
``extract.extract_slide`` refuse the same mask keywords with the same words before a slide is opened, apply the same defaults, and
the command lines' mask flags give the keywords this file writes out."""
import argparse
import inspect

import numpy as np
import pytest

DEFAULTS = dict(cell_mask=None, qc=None, qc_width=2048, qc_fraction=0.6, focus_threshold=None, focus_mpp=4.0, focus_sigma=3.0,
                rois=None, roi_method='auto', roi_filter_method='center', roi_width=2048)

REFUSED = [dict(qc='blur'), dict(qc='both'), dict(qc='otsu', qc_fraction=1.5), dict(qc='otsu', qc_width=0), dict(focus_threshold=-1.0),
           dict(focus_threshold=0.02, focus_sigma=0.0), dict(focus_threshold=0.02, focus_mpp=0.0),
           dict(focus_threshold=0.02, qc_fraction=-0.1), dict(focus_sigma=0.0), dict(roi_method='inside'), dict(roi_method='sideways'),
           dict(roi_filter_method=0.0), dict(roi_filter_method=1.5), dict(roi_filter_method='centre'), dict(roi_width=0),
           dict(rois=[np.array([[0, 0], [10, 10]])]), dict(rois='/nonexistent/rois.csv')]


def _refusal(call):
    with pytest.raises(Exception) as e:
        call()
    return type(e.value), str(e.value)


@pytest.mark.parametrize('kw', REFUSED, ids=lambda kw: ','.join(f'{k}={v}' if np.isscalar(v) else k for k, v in kw.items()))
def test_refusals_alike(tmp_path, kw):
    """Both refuse before the slide is opened (the path does not exist) and before the engine is touched (there is none)."""
    from biscuit_amd.extract import extract_slide
    from biscuit_amd.heatmap import Heatmap
    missing, outdir = str(tmp_path / 'missing.svs'), tmp_path / 'out'
    heat = _refusal(lambda: Heatmap.from_slide(None, missing, **kw))
    extr = _refusal(lambda: extract_slide(None, missing, str(outdir), **kw))
    assert heat == extr and heat[1], (heat, extr)
    assert heat[0] is (FileNotFoundError if kw.get('rois') == '/nonexistent/rois.csv' else ValueError)
    assert not outdir.exists()


def test_defaults():
    from biscuit_amd.extract import extract_slide
    from biscuit_amd.heatmap import Heatmap
    assert len(DEFAULTS) == 11
    for fn in (Heatmap.from_slide, extract_slide):
        params = inspect.signature(fn).parameters
        assert {k: params[k].default for k in DEFAULTS} == DEFAULTS, fn.__qualname__


FLAGS = [([], {}),
         (['--qc-focus'], dict(focus_threshold=0.02)),
         (['--qc-focus', '0.05'], dict(focus_threshold=0.05)),
         (['--qc', 'otsu', '--qc-fraction', '0.4'], dict(qc='otsu', qc_fraction=0.4)),
         (['--qc', 'otsu', '--qc-width', '600', '--qc-focus', '--qc-focus-mpp', '8', '--qc-focus-sigma', '1.5'],
          dict(qc='otsu', qc_width=600, focus_threshold=0.02, focus_mpp=8.0, focus_sigma=1.5)),
         (['--roi-filter', '0.5'], dict(roi_filter_method=0.5)),
         (['--roi-filter', 'center'], dict(roi_filter_method='center')),
         (['--rois', 'F', '--roi-method', 'outside', '--roi-width', '512'], dict(rois='F', roi_method='outside', roi_width=512))]


def _parser():
    from biscuit_amd.slide_input import add_mask_arguments
    ap = argparse.ArgumentParser()
    add_mask_arguments(ap)
    return ap


@pytest.mark.parametrize('argv,want', FLAGS, ids=lambda v: ' '.join(v) or 'none' if isinstance(v, list) else None)
def test_flags(argv, want):
    from biscuit_amd.slide_input import mask_keywords
    ap = _parser()
    got = mask_keywords(ap, ap.parse_args(argv))
    flagged = {k: v for k, v in DEFAULTS.items() if k != 'cell_mask'}                    # (the caller's own mask has no flag)
    assert got == dict(flagged, **want)
    assert all(type(got[k]) is type(v) for k, v in dict(flagged, **want).items()), got


@pytest.mark.parametrize('argv', [['--roi-filter', 'x'], ['--qc', 'blur']], ids=' '.join)
def test_flags_refused(argv, capsys):
    from biscuit_amd.slide_input import mask_keywords
    ap = _parser()
    with pytest.raises(SystemExit) as e:
        mask_keywords(ap, ap.parse_args(argv))
    assert e.value.code == 2 and argv[1] in capsys.readouterr().err
