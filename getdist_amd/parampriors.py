"""
``ParamBounds``: hard prior ranges and periodic flags of the parameters (getdist/parampriors.py).
"""

class ParamBounds:
    """Hard prior ranges and periodic flags (parampriors.py:6-139, the parts the hot path uses)."""

    def __init__(self):
        self.lower, self.upper, self.periodic = {}, {}, set()

    def setRange(self, name, rng):
        lo, hi = rng[0], rng[1]
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

    def fixedValue(self, name):
        lo, hi = self.lower.get(name), self.upper.get(name)
        return lo if lo is not None and lo == hi else None

    def getLower(self, name):
        return self.lower.get(name)

    def getUpper(self, name):
        return self.upper.get(name)
