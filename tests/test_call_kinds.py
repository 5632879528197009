"""CPU, no GPU and no library: the lists of tests/_history.py against what the library exports, so that the circuits cannot fall behind the entry points again.

repaq_amd/csrc/exports.map says which symbols librfq_hip.so exports - "the C entry points of include/rfq_hip.h and nothing else", by pattern - and the header declares
them (RFQ_API).  Every one of them is either called by the step of a kind of call (_history.KIND_ENTRY_POINTS) or listed, with the reason, as no kind of call
(_history.NOT_A_CALL_KIND).  A new entry point fails here by name until it is in one of the two; a name in either that is no longer exported fails too."""
import fnmatch
import os
import re

import _history as H

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _read(*path):
    with open(os.path.join(ROOT, *path)) as f:
        return f.read()


def exported():
    """the names the export map lets out of the library: the header's RFQ_API functions that match one of its `global:` patterns (and none of `local:` first)"""
    text = re.sub(r"/\*.*?\*/", "", _read("repaq_amd", "csrc", "exports.map"), flags=re.S)
    patterns = {sec: [p.strip() for p in body.split(";") if p.strip()] for sec, body in re.findall(r"(global|local)\s*:\s*([^{}]*?)(?=global\s*:|local\s*:|\})", text)}
    assert patterns.get("global") and patterns.get("local") == ["*"], patterns
    header = re.sub(r"/\*.*?\*/", "", _read("include", "rfq_hip.h"), flags=re.S)
    declared = re.findall(r"^RFQ_API\b[^;()]*?\b(\w+)\s*\(", header, flags=re.M)
    assert len(declared) == len(set(declared)) and len(declared) > 40, declared
    names = [n for n in declared if any(fnmatch.fnmatchcase(n, p) for p in patterns["global"])]
    assert names == declared, "the header declares entry points the export map keeps local: %s" % sorted(set(declared) - set(names))
    return names


def test_the_export_map_is_read_as_the_linker_reads_it():
    names = exported()
    assert {"rfq_create", "rfq_encode_batch", "rfq_dedup_rows", "rfq_group_rows", "rfq_version"} <= set(names) and all(n.startswith("rfq_") for n in names)
    # (every definition of an exported function in the sources is one the header declares: nothing is exported behind the header's back)
    defined = set()
    for unit in ("rfq_api.hip", "rfq_encode.hip", "rfq_decode.hip"):
        defined |= set(re.findall(r'^extern "C"[^;(){]*?\b(rfq_\w+)\s*\(', _read("repaq_amd", "csrc", unit), flags=re.M))
    assert defined and defined <= set(names), sorted(defined - set(names))


def test_every_entry_point_is_a_kind_of_call_or_says_why_not():
    names = exported()
    called = {e for eps in H.KIND_ENTRY_POINTS.values() for e in eps}
    aside = [n for n, _ in H.NOT_A_CALL_KIND]
    assert all(len(why.split()) >= 2 for _, why in H.NOT_A_CALL_KIND), "every name of NOT_A_CALL_KIND carries a few words on why"
    assert len(aside) == len(set(aside)) and not called & set(aside), sorted(called & set(aside))
    missing = [n for n in names if n not in called and n not in aside]
    assert not missing, "exported, in no kind's step and not in NOT_A_CALL_KIND: %s" % missing
    gone = sorted((called | set(aside)) - set(names))
    assert not gone, "listed in tests/_history.py and not exported any more: %s" % gone


def test_every_kind_has_its_step_its_batch_and_its_refusal():
    kinds = H.CALL_KINDS
    assert len(kinds) == len(set(kinds)) == 19 and set(H.KIND_ENTRY_POINTS) == set(kinds), sorted(set(H.KIND_ENTRY_POINTS) ^ set(kinds))
    assert all(H.KIND_ENTRY_POINTS[k] for k in kinds)
    for k in kinds + H.REFUSING_CALL_KINDS:
        assert callable(getattr(H.Calls, k, None)), "Calls has no step %s" % k
    assert set(H.CALL_STAGES) <= set(kinds)
    # a small batch behind a large one: every kind, or the reason why its scratch cannot hold anything of a larger call (every rows kind is among the first)
    assert len(H.NOTHING_LEFT_CALLS) == len(set(H.NOTHING_LEFT_CALLS)) == 15 and set(H.NOTHING_LEFT_CALLS) <= set(kinds)
    exempt = [k for k, _ in H.NO_NOTHING_LEFT]
    assert all(len(why.split()) >= 2 for _, why in H.NO_NOTHING_LEFT) and not set(exempt) & set(H.NOTHING_LEFT_CALLS)
    assert sorted(exempt + list(H.NOTHING_LEFT_CALLS)) == sorted(kinds), sorted(set(kinds) - set(exempt) - set(H.NOTHING_LEFT_CALLS))
    rows_kinds = [k for k in kinds if any(re.search(r"rows|names", e) for e in H.KIND_ENTRY_POINTS[k])]
    assert len(rows_kinds) == 15 and set(rows_kinds) == set(H.NOTHING_LEFT_CALLS), sorted(set(rows_kinds) ^ set(H.NOTHING_LEFT_CALLS))
    for k in H.NOTHING_LEFT_CALLS:
        assert callable(getattr(H.Batch, k, None)), "Batch has no call %s" % k
    # a refusal on the device: every kind has a refusing kind, or the reason why it has none
    assert len(H.REFUSING_CALL_KINDS) == len(set(H.REFUSING_CALL_KINDS)) == 18 and set(H.REFUSING_KIND_OF) == set(H.REFUSING_CALL_KINDS)
    refused = set(H.REFUSING_KIND_OF.values()); never = [k for k, _ in H.NO_REFUSING_KIND]
    assert refused <= set(kinds) and all(len(why.split()) >= 2 for _, why in H.NO_REFUSING_KIND) and not refused & set(never)
    assert sorted(refused | set(never)) == sorted(kinds), "neither a refusing kind nor a reason: %s" % sorted(set(kinds) - refused - set(never))
