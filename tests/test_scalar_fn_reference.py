"""CPU: pins the oracle the device tests of the scalar functions use (tests/scalar_fn_reference.py).  It reproduces every known answer of the reference
(tests/golden/scalar_functions.json) and a few hand-written edges per rule; and the C ABI declares the two entry points."""
import datetime

import pytest

import scalar_fn_reference as ref

GOLDENS = ref.load_goldens()
N = None


def test_fixture_holds_the_reference_answers():
    names = [c["name"] for c in GOLDENS]
    assert len(names) == len(set(names)) == 57
    by_fn = {}
    for c in GOLDENS:
        by_fn[c["fn"]] = by_fn.get(c["fn"], 0) + 1
    assert by_fn == {"character_length": 4, "left": 9, "right": 9, "starts_with": 4, "substr": 19, "date_part": 12}
    assert sum("error" in c for c in GOLDENS) == 1
    for c in GOLDENS:
        if c["fn"] == "date_part":
            assert (datetime.date.fromisoformat(c["args"][1]) - datetime.date(1970, 1, 1)).days == c["days"]


@pytest.mark.parametrize("case", GOLDENS, ids=[c["name"] for c in GOLDENS])
def test_reference_reproduces_the_goldens(case):
    args = ref.golden_args(case)
    if "error" in case:
        with pytest.raises(ref.NegativeSubstringLength) as e:
            ref.evaluate(case["fn"], args)
        assert str(e.value).startswith(case["error"])
        return
    got = ref.evaluate(case["fn"], args)
    assert got == case["expected"] and type(got) is type(case["expected"])


def test_date_part_edges():
    day = lambda y, m, d: (datetime.date(y, m, d) - datetime.date(1970, 1, 1)).days
    assert ref.MIN_DAY == day(1, 1, 1) and ref.MAX_DAY == day(9999, 12, 31)
    assert ref.date_part("year", day(1900, 2, 28) + 1) == 1900.0 and ref.date_part("month", day(1900, 2, 28) + 1) == 3.0          # 1900 is no leap year
    assert ref.date_part("day", day(2000, 2, 28) + 1) == 29.0                                                                      # 2000 is one
    assert ref.date_part("doy", day(2000, 12, 31)) == 366.0 and ref.date_part("doy", day(2100, 12, 31)) == 365.0
    assert ref.date_part("week", day(2018, 12, 31)) == 1.0 and ref.date_part("week", day(2020, 12, 31)) == 53.0 and ref.date_part("week", day(2021, 1, 3)) == 53.0
    assert ref.date_part("week", day(2016, 1, 3)) == 53.0 and ref.date_part("week", day(2017, 1, 1)) == 52.0
    assert ref.date_part("dow", day(1970, 1, 1)) == 4.0 and ref.date_part("dow", day(2024, 9, 1)) == 0.0
    assert ref.date_part("quarter", day(2024, 12, 1)) == 4.0 and ref.date_part("QuArTeR", day(2024, 3, 31)) == 1.0
    assert ref.date_part("epoch", -1) == -86400.0 and ref.date_part("hour", 12345) == 0.0
    assert ref.date_part(N, 1) is N and ref.date_part("year", N) is N
    with pytest.raises(ValueError, match="Date part 'fortnight' not supported"):
        ref.date_part("fortnight", 0)


def test_string_edges():
    s = "aä€😀b"
    assert ref.character_length(s) == 5 and len(s.encode()) == 11
    assert ref.substr(s, 2) == "ä€😀b" and ref.substr(s, -7) == s and ref.substr(s, 6) == "" and ref.substr(s, 2**40) == ""
    assert ref.substr(s, 2, 2, True) == "ä€" and ref.substr(s, 0, 2, True) == "a" and ref.substr(s, -1, 2, True) == "" and ref.substr(s, -1, 3, True) == "a"
    assert ref.substr(s, 2, 2**40, True) == "ä€😀b" and ref.substr(s, -2**40, 2**40, True) == "" and ref.substr(s, -2**40, 2**40 + 3, True) == "aä"
    assert ref.substr(s, 1, 0, True) == "" and ref.substr(N, 1, -1, True) is N and ref.substr(s, N, -1, True) is N and ref.substr(s, 1, N, True) is N
    with pytest.raises(ref.NegativeSubstringLength):
        ref.substr(s, 9, -1, True)
    assert ref.left(s, 2) == "aä" and ref.left(s, -2) == "aä€" and ref.left(s, -5) == "" and ref.left(s, -2**40) == "" and ref.left(s, 2**40) == s
    assert ref.right(s, 2) == "😀b" and ref.right(s, -2) == "€😀b" and ref.right(s, -5) == "" and ref.right(s, -2**40) == "" and ref.right(s, 2**40) == s
    assert ref.left("", 1) == "" and ref.right("", -1) == "" and ref.left(s, 0) == "" and ref.right(s, 0) == ""
    assert ref.starts_with(s, "aä") and ref.starts_with(s, "") and not ref.starts_with(s, "ä") and not ref.starts_with("a", "ab") and ref.starts_with("", "")
    assert ref.rows("left", [["ab", N, "cd"], [1, 1, N]]) == ["a", N, N]


def test_c_abi_declares_scalar_function():
    from dfgpu import capi
    assert "dfgpu_scalar_function" in capi.PROTOTYPES and "dfgpu_expr_scalar_function" in capi.PROTOTYPES
    assert len(capi.PROTOTYPES["dfgpu_scalar_function"][1]) == 6 and len(capi.PROTOTYPES["dfgpu_expr_scalar_function"][1]) == 4
    from dfgpu import physical_plan as pp
    assert [pp.FN_DATE_PART, pp.FN_CHARACTER_LENGTH, pp.FN_SUBSTR, pp.FN_LEFT, pp.FN_RIGHT, pp.FN_STARTS_WITH] == [ref.FN[k] for k in ("date_part", "character_length", "substr", "left", "right", "starts_with")]
