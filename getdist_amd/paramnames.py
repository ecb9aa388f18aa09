"""
Parameter names and per-parameter state: ``ParamInfo`` and ``ParamNames``, the parts of getdist/paramnames.py that
the KDE / weighted-statistics path reads and writes, and the list behaviour the result types share with them.
"""

import copy as _copy

try:
    # GetDist's plotting layer -- the caller this package is a drop-in for -- recognises a parameter object by
    # isinstance(param, getdist.paramnames.ParamInfo) (plots.py:607,1981,2027).  Where GetDist is installed beside this
    # package our parameter objects therefore derive from its class; without it they stand alone.
    from getdist.paramnames import ParamInfo as _PlotParamInfo
except Exception:  # noqa: BLE001 -- not installed (or not importable): nothing of the path needs it
    _PlotParamInfo = object


class ParamInfo(_PlotParamInfo):
    """Per-parameter state bag; the attributes the hot path reads and writes (paramnames.py:69-154)."""

    def __init__(self, name="", label=None):
        if _PlotParamInfo is not object:
            super().__init__(name=name, label=label or name)
        self.name = name
        self.label = label or name
        self._label_given = bool(label)  # the reference's label of a parameter without one is "" (what string() writes)
        self.isDerived = False
        self.limmin = self.limmax = None
        self.has_limits_bot = self.has_limits_top = self.has_limits = False
        self.periodic = False
        self.N_eff_kde = None
        self.kde_h = None
        self.renames = []   # alternative names a caller may use for this parameter (paramnames.py:86)
        self.comment = ""

    def getLabel(self):
        """paramnames.py:120-124"""
        return self.label if self.label else self.name

    def latexLabel(self):
        """paramnames.py:126-130: what the plotting layer writes on an axis"""
        return "$" + self.label + "$" if self.label else self.name

    def string(self, wantComments=True):
        """paramnames.py:137-144: the parameter's line of a .paramnames file"""
        res = self.name
        if self.isDerived:
            res += "*"
        res = res + "\t" + (self.label if getattr(self, "_label_given", True) or self.label != self.name else "")
        if wantComments and self.comment != "":
            res = res + "\t#" + self.comment
        return res

    def __str__(self):
        return self.string()

    def __repr__(self):
        return "ParamInfo(%s)" % self.name


class ParamList:
    """The list behaviour shared by ParamNames and the result types of types.py (paramnames.py:156-416, the part they
    use): ``names`` is an ordered list of ParamInfo objects."""

    def __init__(self):
        self.names = []

    def list(self):
        return [p.name for p in self.names]

    def numParams(self):
        return len(self.names)

    def saveAsText(self, filename):
        """paramnames.py:397-404: write str(self) -- the .paramnames file of a ParamNames, the .margestats / .likestats
        text of a result"""
        with open(filename, "w", encoding="utf-8") as f:
            f.write(str(self))

    def fileList(self, fname):
        """paramnames.py:344-347: the lines of a text file (a byte-order mark is dropped)"""
        with open(fname, encoding="utf-8-sig") as f:
            return f.readlines()

    def filteredCopy(self, params):
        """paramnames.py:352-361: a copy restricted to ``params`` (names, or an object listing them).  The copy is deep --
        it shares no parameter object with this one -- and follows the order of ``params``; names not present are left
        out.  (The reference's copy shares the parameter objects and keeps this object's order.)"""
        wanted = params.list() if hasattr(params, "list") else [getattr(p, "name", p) for p in params]
        new = _copy.copy(self)
        new.__dict__ = {k: _copy.deepcopy(v) for k, v in self.__dict__.items() if k != "names"}
        own = {p.name: p for p in self.names}
        new.names = [_copy.deepcopy(own[nm]) for nm in wanted if nm in own]
        return new

    def maxNameLen(self):
        return max(len(p.name) for p in self.names)

    def parFormat(self):
        """paramnames.py:380-382: the %-format of the name column of a result file"""
        return "%-" + str(max(9, self.maxNameLen()) + 1) + "s"

    def name(self, ix, tag_derived=False):
        """paramnames.py:384-389: name of parameter ``ix``, with a * behind a derived one if asked"""
        par = self.names[ix]
        return par.name + "*" if tag_derived and par.isDerived else par.name

    def parWithName(self, name, error=False, renames=None):
        """paramnames.py:232-255: the parameter called ``name`` -- by its own name, by one of its ``renames``, or through the
        optional ``renames`` mapping {name: alternative name(s)} the plotting layer passes along."""
        if not isinstance(name, str):
            raise ValueError('"name" must be a parameter name string not %s: %s' % (type(name), name))

        def alts(key):
            v = renames.get(key, []) if renames else []
            return [v] if isinstance(v, str) else list(v)

        asked = {name, *alts(name)}
        for p in self.names:
            if asked & {p.name, *getattr(p, "renames", []), *alts(p.name)}:
                return p
        if error:
            from .chains import ParamError  # (chains imports this module)

            raise ParamError("parameter name not found: %s" % name)
        return None


class ParamNames(ParamList):
    info_dict = None          # the parsed yaml of a Cobaya run, when the names were loaded from one (paramnames.py:451)
    filenameLoadedFrom = ""   # paramnames.py:436: the file's name without its folder

    def __init__(self, names, labels=None):
        labels = labels or [None] * len(names)
        self.names = [ParamInfo(n, lab) for n, lab in zip(names, labels)]

    @classmethod
    def fromFile(cls, fileName):
        """A ParamNames loaded from a ``.paramnames`` file or from the yaml file of a Cobaya run (loadFromFile)"""
        new = cls([])
        new.loadFromFile(fileName)
        return new

    def loadFromFile(self, fileName):
        """paramnames.py:431-470: replace the parameters by those of a file.

        ``.paramnames``: one ``name[*]  label  [# comment]`` line per parameter (chainfiles.readParamNames).
        ``.yaml`` / ``.yml`` (a Cobaya ``updated.yaml``): the entries of cobaya_interface.get_info_params, the sampled
        parameters first and then the derived ones, each in the order of the file -- the order of the columns of the run's
        chain files; fixed parameters are neither.  The label is the entry's ``latex`` (the name if it has none), renames
        its ``renames``.  The parsed file is kept as ``info_dict``.  Any other suffix raises ValueError."""
        import os

        extension = os.path.splitext(fileName)[-1]
        if extension == ".paramnames":
            from .chainfiles import readParamNames

            names, labels, derived, comments = readParamNames(fileName, with_comments=True)
            self.names = [ParamInfo(n, lab) for n, lab in zip(names, labels)]
            for par, d, c in zip(self.names, derived, comments):
                par.isDerived, par.comment = d, c
        elif extension.lower() in (".yaml", ".yml"):
            from . import cobaya_interface as ci
            from .yaml_tools import yaml_load_file

            self.info_dict = yaml_load_file(fileName)
            entries = ci.get_info_params(self.info_dict)
            self.names = []
            for derived, wanted in ((False, ci.is_sampled_param), (True, ci.is_derived_param)):
                for name, entry in entries.items():
                    if wanted(entry):
                        par = ParamInfo(name, (entry or {}).get(ci._p_label, name))
                        alts = (entry or {}).get(ci._p_renames) or []
                        par.renames = [alts] if isinstance(alts, str) else list(alts)
                        par.isDerived = derived
                        self.names.append(par)
        else:
            raise ValueError("ParanNames must be loaded from .paramnames or .yaml/.yml file, found %s" % fileName)
        self.filenameLoadedFrom = os.path.split(fileName)[1]

    def __str__(self):
        """paramnames.py:391-395"""
        return "".join(par.string() + "\n" for par in self.names)

    def hasParam(self, name):
        return self.numberOfName(name) != -1

    def getMatches(self, pattern, strings=False):
        """paramnames.py:299-307: parameters whose name matches a shell-style pattern"""
        import fnmatch

        return [(p.name if strings else p) for p in self.names if fnmatch.fnmatchcase(p.name, pattern)]

    def parsWithNames(self, names, error=False, renames=None):
        """paramnames.py:273-297: ParamInfo per name (None where a name is unknown and ``error`` is false for it); names
        holding * or ? expand to every match; ``error`` may be one flag or one per name."""
        if isinstance(names, str):
            names = [names]
        flags = list(error) if isinstance(error, (list, tuple)) else [error]
        if len(flags) < len(names):
            flags = len(names) * flags
        out = []
        for nm, flag in zip(names, flags):
            if isinstance(nm, ParamInfo):
                out.append(nm)
            elif "?" in nm or "*" in nm:
                out += self.getMatches(nm)
            else:
                out.append(self.parWithName(nm, flag, renames))
        return out

    def getRenames(self, keep_empty=False):
        """paramnames.py:324-332"""
        return {p.name: list(getattr(p, "renames", [])) for p in self.names if keep_empty or getattr(p, "renames", [])}

    def updateRenames(self, renames):
        """paramnames.py:334-342: merge the mapping {name: alternative name(s)} into the parameters' renames.  Names are
        alternatives of one another when a chain of entries (the parameters' own and the given ones, keys and values
        alike) connects them; every parameter ends up with the other names of its group.  The reference keeps a group in
        a set, so the order of a renames list is not defined there; here a parameter's own renames come first and the new
        ones follow in the order given."""
        groups = [[p.name, *getattr(p, "renames", [])] for p in self.names]
        own = len(groups)
        for key, alt in (renames or {}).items():
            groups.append([key, *([alt] if isinstance(alt, str) else list(alt or []))])
        merged = True
        while merged:  # join groups that share a name until none do
            merged = False
            for a in range(len(groups)):
                for b in range(a + 1, len(groups)):
                    if set(groups[a]) & set(groups[b]):
                        groups[a] += [nm for nm in groups.pop(b) if nm not in groups[a]]
                        own -= b < own
                        merged = True
                        break
                if merged:
                    break
        for group in groups[:own]:  # (two parameters joined into one group: the first one holds the names, as a dict key would)
            par = self.names[self.numberOfName(group[0])]
            par.renames = [nm for nm in group if nm != par.name]

    def labels(self):
        return [p.label for p in self.names]

    def numberOfName(self, name):
        for i, p in enumerate(self.names):
            if p.name == name:
                return i
        return -1

    def numNonDerived(self):
        return len([p for p in self.names if not p.isDerived])

    def deleteIndices(self, indices):
        gone = set(indices)
        self.names = [p for i, p in enumerate(self.names) if i not in gone]
