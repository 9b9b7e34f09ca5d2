"""The Python mirror's size protocol of the table calls (_sized_call), without
a device: stub callables in place of the C entry points.  The codes of the C
side are pinned by test_table_api_contract_gpu.py."""
import pytest

import logparser_amd as lpa

FAMILIES = {
    "select": lpa._SELECT_ERRORS,
    "table_from": lpa._TABLE_FROM_ERRORS,
    "table_device": lpa._TABLE_DEVICE_ERRORS,
    "table_dict": lpa._DICT_ERRORS,
    "table_map": lpa._MAP_ERRORS,
}
# what each family raises for a code, and the message (a code not named: ValueError with the code)
RAISES = {
    ("table_device", lpa.LP_E_UNSUPPORTED): (lpa.FallbackRequired, "a column's values are derived on the host only: use table_from"),
    ("table_dict", lpa.LP_E_UNSUPPORTED): (lpa.FallbackRequired,
                                           "a column's values are derived on the host only: use table_dict_from"),
    ("table_map", lpa.LP_E_UNSUPPORTED): (lpa.FallbackRequired,
                                          "a map column's members are derived on the host only: use table_map_from"),
    ("table_map", lpa.LP_E_MISSING): (lpa.MissingDissectorsException, "lp_result_table_map: a path the parser does not deliver"),
}
PLAIN = {"select": "lp_result_select failed: %d", "table_from": "lp_result_table failed: %d",
         "table_device": "lp_result_table (device) failed: %d", "table_dict": "lp_result_table_dict failed: %d",
         "table_map": "lp_result_table_map failed: %d"}
CODES = (lpa.LP_E_INVALID, lpa.LP_E_MISSING, lpa.LP_E_UNSUPPORTED, lpa.LP_E_DEVICE, lpa.LP_E_STATE)


class Stub:
    """a C entry point that answers the given codes in turn, and the grow() beside it"""

    def __init__(self, *codes):
        self.codes, self.calls, self.grown = list(codes), 0, 0

    def call(self):
        self.calls += 1
        return self.codes.pop(0)

    def grow(self):
        assert self.calls == 1, "grow() comes between the two calls"
        self.grown += 1


@pytest.mark.parametrize("family", sorted(FAMILIES))
def test_ok_first_try(family):
    s = Stub(lpa.LP_OK)
    assert lpa._sized_call(s.call, s.grow, FAMILIES[family]) is None
    assert (s.calls, s.grown) == (1, 0)


@pytest.mark.parametrize("family", sorted(FAMILIES))
def test_nomem_then_ok(family):
    s = Stub(lpa.LP_E_NOMEM, lpa.LP_OK)
    lpa._sized_call(s.call, s.grow, FAMILIES[family])
    assert (s.calls, s.grown) == (2, 1)


@pytest.mark.parametrize("family", sorted(FAMILIES))
def test_nomem_twice_raises(family):
    s = Stub(lpa.LP_E_NOMEM, lpa.LP_E_NOMEM, lpa.LP_OK)
    with pytest.raises(ValueError) as e:
        lpa._sized_call(s.call, s.grow, FAMILIES[family])
    assert type(e.value) is ValueError and str(e.value) == PLAIN[family] % lpa.LP_E_NOMEM
    assert (s.calls, s.grown) == (2, 1)


@pytest.mark.parametrize("code", CODES)
@pytest.mark.parametrize("family", sorted(FAMILIES))
def test_other_codes_raise_after_one_call(family, code):
    exc, msg = RAISES.get((family, code), (ValueError, PLAIN[family] % code))
    for codes in ((code,), (lpa.LP_E_NOMEM, code)):  # on the first call, and on the repeat
        s = Stub(*codes)
        with pytest.raises(exc) as e:
            lpa._sized_call(s.call, s.grow, FAMILIES[family])
        assert type(e.value) is exc and str(e.value) == msg
        assert (s.calls, s.grown) == (len(codes), len(codes) - 1)
