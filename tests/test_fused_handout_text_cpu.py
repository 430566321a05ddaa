"""The problem hand-out of the six persistent fused kernels is written once in csrc/mo_fused_device.h -- except for the pieces that have to stay
spelled out in each kernel (as shared functions they change the register and spill figures of kernels that already spill): the static-rounds
predicate, the chunk size, the static first chunk with the slot-major first problem, the early request and the branch at the loop end.  Nothing else keeps those
copies equal, so this test does: each piece must appear the expected number of times in kkt_fused.hip and kkt_fused_f32.hip, and every
occurrence must be the same text up to white space and trailing comments."""
import os
import re

CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "mini_opt_amd", "csrc")
KERNELS_PER_FILE = 3   # step, linearize, Solve / Iterate

# piece -> (pattern that finds every copy, occurrences per file)
PIECES = {
    "chunk shift": (r"const int chunk_shift = [^;]*;", KERNELS_PER_FILE),
    "static-rounds predicate": (r"const long long waves_all = [^;]*;\s*const bool st_rounds = [^;]*;", KERNELS_PER_FILE),
    "chunk size": (r"auto chunk_for = \[&\]\(long long observed\) -> int \{.*?\};", KERNELS_PER_FILE),
    "first chunk": (r"int chunk = [^;]*;\s*const long long ticket_base = [^;]*;\s*long long p = [^;]*;\s*long long chunk_end = [^;]*;", KERNELS_PER_FILE),
    "early request": (r"const bool last_of_chunk = [^;]*;\s*int next_chunk = 0;\s*unsigned long long next_ticket = 0;\s*if \(last_of_chunk\) \{[^}]*\}",
                      KERNELS_PER_FILE),
    "loop end": (r"if \(last_of_chunk\) \{\s*p = [^}]*\} else \{[^}]*\}", KERNELS_PER_FILE + 1),   # (+ the Solve kernel's skipped problem)
}


def _code(path):
    text = re.sub(r"//[^\n]*", "", open(path).read())
    return re.sub(r"\s+", " ", text)


def test_the_pieces_left_in_the_kernels_are_the_same_text_everywhere():
    sources = {f: _code(os.path.join(CSRC, f)) for f in ("kkt_fused.hip", "kkt_fused_f32.hip")}
    for piece, (pattern, per_file) in PIECES.items():
        copies = []
        for name, code in sources.items():
            found = [re.sub(r"\s+", " ", m).strip() for m in re.findall(pattern, code)]
            assert len(found) == per_file, (piece, name, len(found))
            copies += found
        assert len(set(copies)) == 1, (piece, sorted(set(copies)))


def test_the_kernels_hold_no_policy_of_their_own():
    """What the header owns is called, not restated: no kernel source takes a ticket, makes one uniform or sleeps on its own."""
    for f in ("kkt_fused.hip", "kkt_fused_f32.hip"):
        code = _code(os.path.join(CSRC, f))
        for needle in ("atomicAdd(a.ticket", "s_sleep", "auto take_ticket", "auto uniform64"):
            assert needle not in code, (f, needle)
        assert code.count("chunk_for(") == 2 * KERNELS_PER_FILE   # the first chunk and the early request
        assert code.count("queue_take_ticket(a, st_rounds, next_chunk, p)") == KERNELS_PER_FILE
        assert code.count("queue_ticket_problem(next_ticket, ticket_base)") == KERNELS_PER_FILE + 1
