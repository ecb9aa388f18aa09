"""
YAML input of Cobaya runs (getdist/yaml_tools.py): ``yaml_load`` / ``yaml_load_file`` with the two departures from plain
PyYAML that Cobaya's ``updated.yaml`` files rely on, and ``InputSyntaxError`` for a file that does not parse.

PyYAML is imported when a yaml text is actually read: importing this module, or loading a GetDist-format root, does not
need it.  (The reference imports it with the module, yaml_tools.py:5-9; the error for a missing PyYAML is the same.)
"""

import re


class InputSyntaxError(Exception):
    """Syntax error in YAML input (yaml_tools.py:13-14)."""


# yaml_tools.py:24-37: YAML 1.1 floats, but the exponent needs no sign and the mantissa no dot -- "1e2" is 100.0
_FLOAT = re.compile(r"""^(?:
     [-+]?[0-9][0-9_]*\.[0-9_]*(?:[eE][-+]?[0-9]+)?
    |[-+]?[0-9][0-9_]*[eE][-+]?[0-9]+
    |\.[0-9_]+(?:[eE][-+][0-9]+)?
    |[-+]?[0-9][0-9_]*(?::[0-5]?[0-9])+\.[0-9_]*
    |[-+]?\.(?:inf|Inf|INF)
    |\.(?:nan|NaN|NAN))$""", re.VERBOSE)
_CONTEXT_LINES = 4


def _yaml():
    try:
        import yaml
    except ModuleNotFoundError:
        raise ModuleNotFoundError("You need to install 'PyYAML' in order to load Cobaya samples.") from None
    return yaml


def _loader(yaml):
    class ScientificLoader(yaml.Loader):
        pass

    ScientificLoader.add_implicit_resolver("tag:yaml.org,2002:float", _FLOAT, list("-+0123456789."))
    # yaml_tools.py:39-43: a Python object named in the file (a likelihood class, a function) loads as None
    ScientificLoader.add_multi_constructor("tag:yaml.org,2002:python/name:", lambda _loader, _suffix, _node: None)
    return ScientificLoader


def yaml_load(text, file_name=None):
    """yaml_tools.py:20-74: the object a YAML text holds.  Scalars such as ``1e2`` (no dot, no exponent sign) are floats and
    ``!!python/name:`` tags give None.  A text that does not parse raises InputSyntaxError naming the file, the line and the
    column (both counted from 1), followed by the lines around the place with the offending one marked."""
    yaml = _yaml()
    try:
        return yaml.load(text, _loader(yaml))
    except yaml.YAMLError as e:
        where = "Error in your input file " + ("'%s'" % file_name if file_name else "")
        mark = getattr(e, "problem_mark", None)
        if mark is None:
            raise InputSyntaxError(where) from None
        line, column = mark.line + 1, mark.column + 1
        lines = text.split("\n")
        margin = " " * 5 + "|"
        shown = [margin + s for s in lines[max(line - 1 - _CONTEXT_LINES, 0):line - 1]]
        shown.append(" --> |" + lines[line - 1] + "    <---- column %d" % column)
        shown += [margin + s for s in lines[line:line + _CONTEXT_LINES]]
        raise InputSyntaxError("%s at line %d, column %d.\n%s\nMaybe inconsistent indentation, '=' instead of ':', no space "
                               "after ':', or a missing ':' on an empty group?" % (where, line, column, "\n".join(shown))) from None


def yaml_load_file(path):
    """yaml_tools.py:77-81: yaml_load of a file's text (utf-8, a byte-order mark is dropped)."""
    with open(path, encoding="utf-8-sig") as f:
        text = f.read()
    return yaml_load(text, file_name=path)
