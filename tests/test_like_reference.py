"""CPU: pins the oracle the device tests of LIKE use (tests/like_reference.py).  like_rows reproduces every known answer of the reference
(tests/golden/like_expr.json) and a table of hand-written cases, one group per rule of the semantics; and the C ABI declares the two entry points."""
import pytest

from like_reference import check_golden, golden_patterns, like_rows, load_goldens

GOLDENS = load_goldens()
N = None

# (value, pattern, LIKE, ILIKE); NOT LIKE / NOT ILIKE are the negations
EDGES = [
    # % matches any run, the empty run included; the match is anchored at both ends
    ("abc", "%", True, True), ("", "%", True, True), ("abc", "%%", True, True), ("abc", "a%", True, True), ("abc", "%c", True, True), ("abc", "%b%", True, True),
    ("abc", "b%", False, False), ("abc", "%b", False, False), ("abc", "a%c", True, True), ("ac", "a%c", True, True), ("abc", "ab", False, False), ("abc", "bc", False, False),
    ("abc", "abc", True, True), ("abc", "abcd", False, False), ("abc", "%abcd%", False, False),
    # the empty pattern matches only the empty string
    ("", "", True, True), ("a", "", False, False), ("", "a", False, False), ("", "_", False, False),
    # _ is one Unicode scalar, not one byte; a line feed too
    ("aäb", "a_b", True, True), ("aäb", "a__b", False, False), ("ä", "_", True, True), ("ä", "__", False, False), ("a\nb", "a_b", True, True), ("\n", "_", True, True),
    ("a\nb", "a%b", True, True), ("a\n", "a", False, False), ("日本語", "___", True, True), ("日本語", "_本_", True, True), ("日本語", "%本%", True, True), ("ab", "_%_", True, True), ("a", "_%_", False, False),
    # escapes: a backslash in front of % or _ is that literal character
    ("a%b", "a\\%b", True, True), ("axb", "a\\%b", False, False), ("a_b", "a\\_b", True, True), ("axb", "a\\_b", False, False), ("100%", "%\\%", True, True), ("100", "%\\%", False, False),
    # a backslash in front of anything else, or ending the pattern, is a literal backslash and the next character is read normally
    ("a\\b", "a\\b", True, True), ("ab", "a\\b", False, False), ("a\\", "a\\", True, True), ("a", "a\\", False, False), ("a\\\\b", "a\\\\b", True, True), ("a\\b", "a\\\\b", False, False),
    ("a\\xyz", "a\\%", False, False), ("a\\xyz", "a\\x%", True, True), ("a%", "a\\%", True, True), ("a\\%", "a\\\\%", True, True), ("a\\\\zz", "a\\\\%", False, False), ("a\\", "a\\\\%", False, False),
    # everything else matches itself byte for byte: regex metacharacters are plain, case matters under LIKE
    ("a.c", "a.c", True, True), ("abc", "a.c", False, False), ("a*", "a*", True, True), ("(a)", "(a)", True, True), ("[a]", "[a]", True, True), ("a", "[a]", False, False), ("a$", "a$", True, True),
    ("ABC", "abc", False, True), ("abc", "ABC", False, True), ("aBc", "%b%", False, True), ("PROMO BRUSHED", "promo%", False, True),
    # ILIKE: ASCII letters fold; k and s also match the Kelvin sign and the long s; non-ASCII letters of the VALUE do not fold against anything
    ("K", "k", False, True), ("K", "K", False, True), ("ſ", "s", False, True), ("ſ", "S", False, True), ("aKb", "%k%", False, True), ("ſt", "st", False, True),
    ("Ä", "a", False, False), ("K", "_", True, True), ("Kx", "k_", False, True),
    # length limits: a pattern longer than the row, prefix and suffix that would overlap
    ("ab", "ab%b", False, False), ("abb", "ab%b", True, True), ("aba", "aba%aba", False, False), ("abaaba", "aba%aba", True, True), ("a", "a%a", False, False), ("aa", "a%a", True, True),
    # overlapping segments: leftmost-first, each segment behind the one in front
    ("aXa", "%aX%Xa%", False, False), ("aXXa", "%aX%Xa%", True, True), ("aaa", "%aa%aa%", False, False), ("aaaa", "%aa%aa%", True, True), ("abab", "%ab%ab", True, True), ("aba", "%ab%ba", False, False),
    ("special packages requests", "%special%requests%", True, True), ("requests special", "%special%requests%", False, False),
]


def test_fixture_holds_the_reference_answers():
    names = [c["name"] for c in GOLDENS]
    assert names[:4] == ["like_op_like", "like_op_not_like", "like_op_ilike", "like_op_not_ilike"]
    assert sum(n.startswith("strings_") for n in names) == 5
    assert len(names) == len(set(names)) == 22


@pytest.mark.parametrize("case", GOLDENS, ids=[c["name"] for c in GOLDENS])
def test_like_rows_reproduces_the_reference(case):
    patterns, _ = golden_patterns(case)
    check_golden(case, like_rows(case["values"], patterns, case["negated"], case["case_insensitive"]))


@pytest.mark.parametrize("value,pattern,like,ilike", EDGES, ids=[f"{i}" for i in range(len(EDGES))])
def test_like_rows_edge_cases(value, pattern, like, ilike):
    assert like_rows([value], pattern) == [like]
    assert like_rows([value], pattern, negated=True) == [not like]
    assert like_rows([value], [pattern], case_insensitive=True) == [ilike]
    assert like_rows([value], [pattern], negated=True, case_insensitive=True) == [not ilike]


def test_like_rows_nulls():
    assert like_rows(["a", N, "b"], "a") == [True, N, False]
    assert like_rows(["a", N, "b"], N) == [N, N, N]
    assert like_rows(["a", N, "b"], N, negated=True) == [N, N, N]
    assert like_rows(["a", "a", N], ["a", N, "a"], negated=True) == [False, N, N]
    assert like_rows([], "a") == []


def test_c_abi_declares_like():
    from dfgpu import capi
    assert "dfgpu_like" in capi.PROTOTYPES and "dfgpu_expr_like" in capi.PROTOTYPES
    assert len(capi.PROTOTYPES["dfgpu_like"][1]) == 7 and len(capi.PROTOTYPES["dfgpu_expr_like"][1]) == 5
