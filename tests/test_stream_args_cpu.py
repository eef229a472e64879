"""Every launch, asynchronous copy or fill, event call and rocPRIM call in csrc/ names the stream it was handed: the stream
argument is present, is an identifier or a member expression (optionally behind a ``(hipStream_t)`` cast), and is none of
0, nullptr, NULL, hipStreamDefault.  The sources are read as text with a bracket-matching scanner (calls span lines and sit
in macros), comments and string literals removed first.  The number of calls found per kind is recorded below, so a call
written in a form the scanner does not see changes a count instead of slipping past.

rocPRIM calls whose first argument is ``nullptr`` only ask for the size of the temporary storage and launch nothing; they are
counted apart and not checked.  Nothing but stream arguments is looked for here."""
import os
import re

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(os.path.dirname(HERE), "3d-semantic-segmentation_amd", "csrc")

# kind -> index of the stream argument (None: the last argument)
STREAM_ARG = {
    "hipLaunchKernelGGL": 4,        # kernel, grid, block, lds, STREAM, args...
    "hipMemsetAsync": 3,            # dst, value, bytes, STREAM
    "hipMemcpyAsync": 4,            # dst, src, bytes, kind, STREAM
    "hipEventRecord": 1,            # event, STREAM
    "hipStreamWaitEvent": 0,        # STREAM, event, flags
    "rocprim": None,                # ..., STREAM  (debug_synchronous is never passed)
}

# calls found per kind in csrc/*.h and csrc/voxproj.hip; "rocprim_size_query" are the nullptr-first calls that are not checked
RECORDED = {
    "hipLaunchKernelGGL": 97,
    "hipMemsetAsync": 12,
    "hipMemcpyAsync": 6,
    "hipEventRecord": 4,
    "hipStreamWaitEvent": 2,
    "rocprim": 7,
    "rocprim_size_query": 7,
}

FORBIDDEN = {"0", "nullptr", "NULL", "hipStreamDefault"}
STREAM_EXPR = re.compile(r"^(?:\(\s*hipStream_t\s*\)\s*)?[A-Za-z_]\w*(?:\s*(?:\.|->)\s*[A-Za-z_]\w*)*$")
CALL_HEAD = re.compile(r"\b(hipLaunchKernelGGL|hipMemsetAsync|hipMemcpyAsync|hipEventRecord|hipStreamWaitEvent|rocprim::\w+)\s*\(")


def sources():
    names = sorted(f for f in os.listdir(CSRC) if f == "voxproj.hip" or f.endswith(".h"))
    assert "voxproj.hip" in names and len(names) > 20
    return [os.path.join(CSRC, f) for f in names]


def strip_comments_and_strings(text):
    """The text with // and /* */ comments blanked and the inside of string and character literals removed; newlines stay, so
    offsets still map to line numbers.  Line continuations become spaces."""
    out, i, n = [], 0, len(text)
    while i < n:
        c = text[i]
        two = text[i:i + 2]
        if two == "//":
            j = text.find("\n", i)
            j = n if j < 0 else j
            while j < n and text[j - 1] == "\\":                # a continued // comment
                k = text.find("\n", j + 1)
                j = n if k < 0 else k
            out.append(re.sub(r"[^\n]", " ", text[i:j]))
            i = j
        elif two == "/*":
            j = text.find("*/", i + 2)
            j = n if j < 0 else j + 2
            out.append(re.sub(r"[^\n]", " ", text[i:j]))
            i = j
        elif c in "\"'":
            j = i + 1
            while j < n and text[j] != c:
                j += 2 if text[j] == "\\" else 1
            out.append(c + re.sub(r"[^\n]", " ", text[i + 1:j]) + c)
            i = j + 1
        elif two == "\\\n":
            out.append(" \n")
            i += 2
        else:
            out.append(c)
            i += 1
    return "".join(out)


def split_arguments(text, open_paren):
    """The top-level arguments of the call whose '(' is at ``open_paren``, and the offset behind its ')'.  Round, square and
    curly brackets nest; angle brackets are not brackets here (every template-id with a comma in these sources is inside
    round brackets, as the launch macro itself needs)."""
    closing = {"(": ")", "[": "]", "{": "}"}
    stack, args, start = [], [], open_paren + 1
    i = open_paren
    while i < len(text):
        c = text[i]
        if c in closing:
            stack.append(closing[c])
        elif c in ")]}":
            assert stack and stack[-1] == c, f"unbalanced '{c}' at offset {i}"
            stack.pop()
            if not stack:
                args.append(text[start:i])
                return [" ".join(a.split()) for a in args], i + 1
        elif c == "," and len(stack) == 1:
            args.append(text[start:i])
            start = i + 1
        i += 1
    raise AssertionError(f"call at offset {open_paren} never closes")


def find_calls(text):
    """(kind, name, line, arguments) of every call in ``text`` (already stripped), nested ones included."""
    calls = []
    for m in CALL_HEAD.finditer(text):
        name = m.group(1)
        args, _ = split_arguments(text, m.end() - 1)
        kind = "rocprim" if name.startswith("rocprim::") else name
        calls.append((kind, name, text.count("\n", 0, m.start()) + 1, args))
    return calls


def stream_argument(kind, args):
    idx = STREAM_ARG[kind]
    if idx is None:
        return args[-1] if args else None
    return args[idx] if len(args) > idx else None


def stream_fault(kind, args):
    """None when the call's stream argument is acceptable, else what is wrong with it."""
    s = stream_argument(kind, args)
    if s is None or s == "":
        return "no stream argument"
    bare = re.sub(r"^\(\s*hipStream_t\s*\)\s*", "", s)
    if bare in FORBIDDEN:
        return f"stream argument is {s}"
    if not STREAM_EXPR.match(s):
        return f"stream argument '{s}' is not an identifier or member expression"
    return None


@pytest.fixture(scope="module")
def all_calls():
    found = []
    for path in sources():
        with open(path, encoding="utf-8") as f:
            text = strip_comments_and_strings(f.read())
        found += [(os.path.basename(path),) + c for c in find_calls(text)]
    return found


def test_the_scanner_sees_calls_across_lines_macros_casts_and_comments():
    text = strip_comments_and_strings(
        "// hipLaunchKernelGGL(k, g, b, 0, 0)\n"
        "#define GO(K) hipLaunchKernelGGL((K<int, 4>), dim3(f(a, b)), dim3(256), 0, c.s0, x, \\\n    y)\n"
        "hipLaunchKernelGGL(k, g, b, 0,\n   (hipStream_t)stream_, p[i, j]);\n"
        "/* hipMemsetAsync(p, 0, 4, 0); */ VP_HIP(hipMemsetAsync(p, ',', n, stream));\n"
        "rocprim::inclusive_scan(nullptr, bytes, a, b, n, rocprim::plus<int>());\n"
        "VP_HIP(rocprim::inclusive_scan(tmp, bytes, a, b, n, rocprim::plus<int>(), stream));\n"
        "hipLaunchKernelGGL(k, g, b, 0, (hipStream_t)0, p);\nhipMemcpyAsync(d, s, n, kind);\nhipEventRecord(e, nullptr);\n"
        "hipLaunchKernelGGL(k, g, b, 0, pick(s), p);\n")
    calls = find_calls(text)
    assert [(c[0], c[2]) for c in calls] == [
        ("hipLaunchKernelGGL", 2), ("hipLaunchKernelGGL", 4), ("hipMemsetAsync", 6), ("rocprim", 7), ("rocprim", 8),
        ("hipLaunchKernelGGL", 9), ("hipMemcpyAsync", 10), ("hipEventRecord", 11), ("hipLaunchKernelGGL", 12)]
    assert [stream_argument(c[0], c[3]) for c in calls[:3]] == ["c.s0", "(hipStream_t)stream_", "stream"]
    assert calls[3][3][0] == "nullptr" and calls[4][3][0] == "tmp" and calls[4][3][-1] == "stream"
    assert [stream_fault(c[0], c[3]) for c in calls[:3] + calls[4:5]] == [None] * 4
    assert stream_fault(*calls[5][0::3]) == "stream argument is (hipStream_t)0"
    assert stream_fault(*calls[6][0::3]) == "no stream argument"
    assert stream_fault(*calls[7][0::3]) == "stream argument is nullptr"
    assert "not an identifier" in stream_fault(*calls[8][0::3])
    for bad in ("0", "NULL", "hipStreamDefault", "(hipStream_t) 0", "stream + 1", "0 ? a : b", "streams[0]"):
        assert stream_fault("hipEventRecord", ["e", bad]) is not None, bad
    for good in ("s", "c.s0", "ps->side", "c.rec->pipe.s1", "(hipStream_t)stream_"):
        assert stream_fault("hipEventRecord", ["e", good]) is None, good


def test_every_call_in_csrc_names_a_stream(all_calls):
    faults = []
    for fname, kind, name, line, args in all_calls:
        if kind == "rocprim" and args and args[0] == "nullptr":
            continue
        fault = stream_fault(kind, args)
        if fault:
            faults.append(f"{fname}:{line}: {name}: {fault}")
    assert not faults, "\n".join(faults)


def test_the_number_of_calls_of_every_kind_is_the_recorded_one(all_calls):
    found = {k: 0 for k in RECORDED}
    for _, kind, _, _, args in all_calls:
        if kind == "rocprim" and args and args[0] == "nullptr":
            kind = "rocprim_size_query"
        found[kind] += 1
    assert found == RECORDED, "a call was added, removed or written in a form the scanner does not see: check it, then record the count"


def test_no_launch_is_written_with_chevrons():
    """The scanner reads hipLaunchKernelGGL only: a <<< >>> launch would be a form it does not see."""
    for path in sources():
        with open(path, encoding="utf-8") as f:
            assert "<<<" not in strip_comments_and_strings(f.read()), path
