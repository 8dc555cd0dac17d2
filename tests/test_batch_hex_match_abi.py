"""The batch's own match classes (yr_amd_scanner_set_batch_match_classes)
without a GPU: the symbol in the library, the header and the prototypes, its
behaviour on a null scanner, and what the header says of batches."""
import os
import re

import yara_amd
from yara_amd import _lib
from conftest import REPO

NAME = "yr_amd_scanner_set_batch_match_classes"
LIT, HEX = 1, 2


def header():
    with open(os.path.join(REPO, "include", "yara_amd.h")) as f:
        return f.read()


def test_symbol():
    L = _lib.lib()
    assert hasattr(L, NAME)
    assert NAME in _lib.PROTOTYPES
    assert _lib.PROTOTYPES[NAME] == _lib.PROTOTYPES["yr_amd_scanner_set_match_classes"]
    assert re.search(r"\bint %s\(\s*yr_amd_scanner\* scanner,\s*uint32_t classes\);" % NAME, header())
    assert callable(getattr(yara_amd.Scanner, "set_batch_match_classes"))


def test_null_scanner():
    L = _lib.lib()
    for classes in (LIT, LIT | HEX, 0, HEX, 4):
        assert L.yr_amd_scanner_set_batch_match_classes(None, classes) == yara_amd.INVALID_ARGUMENT


def test_header_no_longer_says_literal_only():
    """The YR_AMD_MATCH_HEX section said that the batch calls "ignore the setting
    and stay literal-only"; they ignore THAT setting and have their own."""
    text = " ".join(re.sub(r"^\s*\*", " ", line) for line in header().splitlines())
    text = re.sub(r"\s+", " ", text)
    assert "stay literal-only" not in text
    assert "ignore the setting and stay" not in text
    at = text.index("yr_amd_scanner_set_match_classes: the LITERAL bit must stay set")
    section = text[at:text.index("#define YR_AMD_MATCH_LITERAL")]
    assert NAME in section                       # the hex section points to the batch's setting
    # and the new section states the semantics
    own = text[text.index("Final matches of hex strings in a batch"):]
    own = own[:own.index("int %s(" % NAME)]
    for phrase in ("yr_amd_scan_block_matches(data_k, size_k, bases[k])", "first record in record order",
                   "No byte of a gap", "never a window", "yr_amd_tables_set_re_code",
                   "YR_AMD_MATCH_MAX_RECORDS"):
        assert phrase in own, phrase
