"""The memory-contract manifest (tests/memcheck.py) against include/mliis_hip.h: every entry point the header declares is either
COVERED by a poisoned-memory case or EXEMPT with a reason, and the cases of the GPU modules together declare exactly COVERED.
A new entry point without a memory-contract case fails here, without a GPU."""
import memcheck
import test_abi
import test_memory_contract_gpu as MC
import test_step_poisoned_gpu as SP


def test_manifest_is_exactly_the_header():
    decls = set(test_abi._decls())
    covered, exempt = set(memcheck.COVERED), set(memcheck.EXEMPT)
    assert not covered & exempt, sorted(covered & exempt)
    assert covered | exempt == decls, "not in the manifest: {}; not in the header: {}".format(
        sorted(decls - covered - exempt), sorted((covered | exempt) - decls))
    for name, reason in memcheck.EXEMPT.items():
        assert isinstance(reason, str) and len(reason.strip()) >= 10, name


def test_cases_declare_exactly_the_covered_set():
    declared = set()
    for reach in list(MC.REACHES.values()) + list(SP.REACHES.values()):
        declared |= set(reach)
    assert declared <= set(memcheck.COVERED), sorted(declared - set(memcheck.COVERED))
    assert declared == set(memcheck.COVERED), "COVERED but reached by no case: {}".format(sorted(set(memcheck.COVERED) - declared))
