"""The argument behaviour of every image entry point, replayed from tests/golden/image_call_defects.json (recorded by
tests/golden/make_image_call_defects.py before the calls' host side was gathered into csrc/image_host.h): each defect of each call
alone, every pair of defects, and the calls with nothing to do must give the recorded return code and the recorded
dxtlt_last_error text, byte for byte.  No GPU: every case fails a check or has nothing to do."""
import importlib.util
import json
import os

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def maker():
    spec = importlib.util.spec_from_file_location("make_image_call_defects", os.path.join(GOLDEN, "make_image_call_defects.py"))
    module = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(module)
    return module


def test_every_recorded_return_code_and_error_text(pkg):
    make = maker()
    with open(make.TABLE) as f:
        want = json.load(f)
    rows = make.run(make.load(pkg._lib.lib_path()))
    # case by case first, so that a failure names the case; then the whole table, which also finds a case that is new or gone
    answer_of = make.answers_of(want)
    different = [(call, case, make.answer(rc, text), answer_of.get((call, case))) for call, case, rc, text in rows]
    different = [d for d in different if d[2] != d[3]]
    assert not different, different[:10]
    assert make.table_of(rows) == want, "the cases are not the recorded ones: the table is out of date"
    # the table covers every entry point of the five files, and every kind of answer
    assert set(want) == set(make.SIGNATURES) and {r[2] for r in rows} == {0, 1, 2, -1}
