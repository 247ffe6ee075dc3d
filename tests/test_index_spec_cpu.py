"""Text-level: build_index takes (ctx, index, points, n, IndexSpec) and nothing else; the eleven-parameter positional form, whose
calls nobody could read, does not come back."""
import os
import re

CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "threecrate_amd", "csrc")


def _calls(text, name):
    """the top-level argument lists of every `name(` in text"""
    for m in re.finditer(r"\b" + name + r"\(", text):
        depth, args, start = 1, [], m.end()
        for i in range(m.end(), len(text)):
            c = text[i]
            depth += c in "([{"
            depth -= c in ")]}"
            if depth == 0 or (depth == 1 and c == ","):
                args.append(text[start:i].strip())
                start = i + 1
            if depth == 0:
                break
        yield args


def test_the_call_parser_counts_top_level_arguments():
    text = "x = build_index(ctx, ix, f(a, b), n, knn_grid(k)); build_index(a, b[1, 2], (c, d), e, f, g);"
    assert [len(a) for a in _calls(text, "build_index")] == [5, 6]


def test_build_index_is_called_with_a_spec_everywhere():
    seen = 0
    for f in sorted(os.listdir(CSRC)):
        if not f.endswith((".hip", ".h")):
            continue
        text = re.sub(r"//[^\n]*", "", open(os.path.join(CSRC, f)).read())          # (comments name it as build_index(strict_order))
        for args in _calls(text, "build_index"):
            seen += 1
            assert len(args) == 5, (f, args)
    assert seen >= 14          # twelve calls, the declaration and the definition
