"""
``ParamBounds``: hard prior ranges and periodic flags of the parameters (getdist/parampriors.py).
"""

class ParamBounds:
    """Hard prior ranges and periodic flags (parampriors.py:6-139, the parts the hot path uses)."""

    def __init__(self, fileName=None):
        self.lower, self.upper, self.periodic = {}, {}, set()
        self.names = []  # in the order the ranges were first set: the order of the lines of a .ranges file
        if fileName is not None:
            self.loadFromFile(fileName)

    def loadFromFile(self, fileName):
        """parampriors.py:27-43: add the ranges of a file.

        ``.ranges`` / ``.bounds``: ``name  lower  upper  [periodic]`` lines, ``N`` for an open side (chainfiles.readRanges).
        ``.yaml`` / ``.yml`` (a Cobaya ``updated.yaml``): cobaya_interface.get_range of every entry of get_info_params, so
        the fixed parameters -- which no chain column holds -- come in as zero-width ranges.  Any other suffix raises
        ValueError."""
        import os

        extension = os.path.splitext(fileName)[-1]
        if extension in (".ranges", ".bounds"):
            from .chainfiles import readRanges

            for name, rng in readRanges(fileName).items():
                self.setRange(name, rng)
        elif extension in (".yaml", ".yml"):
            from .cobaya_interface import get_info_params, get_range

            for name, entry in get_info_params(fileName).items():
                self.setRange(name, get_range(entry))
        else:
            raise ValueError("ParamBounds must be loaded from .bounds, .ranges or .yaml/.yml file, not %s" % fileName)
        self.filenameLoadedFrom = os.path.split(fileName)[1]

    def __str__(self):
        """parampriors.py:45-63: one line per parameter, ``%22s%17s%17s`` of name, lower, upper (``%15.7E``, or N for an open
        side), and ``periodic`` behind a periodic one"""
        s = ""
        for name in self.names:
            lo, hi = self.getLower(name), self.getUpper(name)
            lim1 = "%15.7E" % lo if lo is not None else "    N"
            lim2 = "%15.7E" % hi if hi is not None else "    N"
            if name in self.periodic:
                s += "%22s%17s%17s%10s\n" % (name, lim1, lim2, "periodic")
            else:
                s += "%22s%17s%17s\n" % (name, lim1, lim2)
        return s

    def saveToFile(self, fileName):
        """parampriors.py:65-72: write the .ranges file"""
        with open(fileName, "w", encoding="utf-8") as f:
            f.write(str(self))

    def setRange(self, name, rng):
        lo, hi = rng[0], rng[1]
        if not (lo is None and hi is None) and name not in self.names:  # parampriors.py:82-83, 98-99
            self.names.append(name)
        if len(rng) > 2 and rng[2] in (True, "periodic"):
            self.periodic.add(name)
        elif name in self.periodic:
            self.periodic.discard(name)
        for store, v in ((self.lower, lo), (self.upper, hi)):
            if v is None or (isinstance(v, str) and v in ("N", "None")):
                store.pop(name, None)
            else:
                store[name] = float(v)

    def setFixed(self, name, value):
        """parampriors.py:78-79: a fixed parameter is a zero-width range"""
        self.lower[name] = self.upper[name] = float(value)
        if name not in self.names:
            self.names.append(name)

    def fixedValue(self, name):
        lo, hi = self.lower.get(name), self.upper.get(name)
        return lo if lo is not None and lo == hi else None

    def fixedValueDict(self):
        """parampriors.py:130-139: {name: value} of the zero-width ranges"""
        return {name: self.fixedValue(name) for name in self.names if self.fixedValue(name) is not None}

    def getLower(self, name):
        return self.lower.get(name)

    def getUpper(self, name):
        return self.upper.get(name)
