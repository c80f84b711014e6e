"""``extract_slide(img_format=...)`` and ``--img-format`` where no device is needed: the refusals, which come before a slide is
opened or an engine is made.  The extraction itself: tests/test_gpu_extract_png.py."""
import inspect

import pytest

from biscuit_amd import extract


def test_img_format_is_checked_before_the_slide_is_opened(tmp_path):
    for bad in ('jpeg', 'PNG', None, 'tiff'):
        with pytest.raises(ValueError, match='img_format'):
            extract.extract_slide(None, str(tmp_path / 'missing.svs'), str(tmp_path / 'out'), img_format=bad)
    assert not (tmp_path / 'out').exists()
    assert extract.IMG_FORMATS == ('jpg', 'png')
    assert inspect.signature(extract.extract_slide).parameters['img_format'].default == 'jpg'


@pytest.mark.parametrize('extra', [['--quality', '90'], ['--subsampling', '4:4:4'], ['--quality', '95', '--subsampling', '4:2:0']])
def test_jpeg_settings_with_png_are_an_argparse_error(tmp_path, capsys, extra):
    with pytest.raises(SystemExit) as e:
        extract.main([str(tmp_path / 'missing.svs'), '--out', str(tmp_path / 'out'), '--img-format', 'png'] + extra)
    assert e.value.code == 2 and 'jpg only' in capsys.readouterr().err
    assert not (tmp_path / 'out').exists()


def test_an_unknown_format_is_an_argparse_error(tmp_path, capsys):
    with pytest.raises(SystemExit) as e:
        extract.main([str(tmp_path / 'missing.svs'), '--out', str(tmp_path / 'out'), '--img-format', 'jpeg'])
    assert e.value.code == 2 and 'img-format' in capsys.readouterr().err
