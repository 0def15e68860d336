"""The stop-rule and decode-kind codes of codes/schemes.py are the enums of the native runtime
(csrc/runtime/collector.h RuleKind, csrc/runtime/decode.h DecodeKind), exported by the binding."""
from erasurehead_amd.codes import schemes

NAMES = ["RULE_ALL", "RULE_COUNT", "RULE_FRC", "RULE_PARTIAL_FRC", "RULE_PARTIAL_COUNT",
         "DEC_SUM", "DEC_FIRST_PER_GROUP", "DEC_PARTIAL_FRC", "DEC_TABLE", "DEC_PARTIAL_TABLE"]


def test_scheme_codes_equal_the_native_enums(native):
    for name in NAMES:
        assert getattr(schemes, name) == getattr(native, name), name
    for prefix in ("RULE_", "DEC_"):  # no code on either side that the other lacks
        assert sorted(n for n in dir(schemes) if n.startswith(prefix)) == \
            sorted(n for n in dir(native) if n.startswith(prefix)) == sorted(n for n in NAMES if n.startswith(prefix))
