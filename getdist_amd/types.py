"""
Result types of the marginalised and likelihood statistics: ``ParamLimit``, ``MargeStats``, ``LikeStats``
(getdist/types.py, the numbers only).
"""

class ParamLimit:
    """A marginalised parameter limit (types.py:652-716): lower, upper and which tails are constrained."""

    def __init__(self, minmax, tag="two"):
        self.lower, self.upper = minmax[0], minmax[1]
        self.twotail = tag == "two"
        self.onetail_upper = tag == ">"
        self.onetail_lower = tag == "<"

    def limitTag(self):
        return "two" if self.twotail else (">" if self.onetail_upper else ("<" if self.onetail_lower else "none"))

    def __str__(self):
        return f"{self.lower:g} {self.upper:g} {self.limitTag()}"


class MargeStats:
    """The numbers of types.MargeStats (types.py:718-800): per-parameter mean, err and limits per contour."""

    def __init__(self, names, limits):
        self.names = names
        self.limits = limits
        self.hasBestFit = False

    def parWithName(self, name):
        for p in self.names:
            if p.name == name:
                return p
        return None


class LikeStats:
    """The numbers of types.LikeStats (types.py:900-939): posterior statistics of the sample log-likelihoods; the N-D
    confidence-region limits and the best-fit sample live on ``names[i]`` (ND_limit_bot / ND_limit_top / bestfit_sample)."""

    def __init__(self):
        self.logLike_sample = self.logMeanInvLike = self.meanLogLike = self.logMeanLike = None
        self.complexity = self.varLogLike = None
        self.names = []

    def likeSummary(self):
        text = "Best fit sample -log(Like) = %f\n" % self.logLike_sample
        if self.logMeanInvLike:
            text += "Ln(mean 1/like) = %f\n" % self.logMeanInvLike
        text += "mean(-Ln(like)) = %f\n" % self.meanLogLike
        text += "-Ln(mean like)  = %f\n" % self.logMeanLike
        text += "2*Var(Ln(like)) = %f\n" % (self.varLogLike * 2.0)
        return text
