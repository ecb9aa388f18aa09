"""
Result types and the text a person reads from them (getdist/types.py): number formatting to significant figures,
LaTeX table formatters, ``ResultTable``, and ``ParamLimit`` / ``MargeStats`` / ``LikeStats`` with their text forms.

Everything here works on the ten or so doubles per parameter that getMargeStats / getLikeStats bring back from the
device; nothing in this module calls the device.  Not rebuilt: ``ResultTable.tablePNG`` (it runs latex and dvipng),
``BestFit`` / ``MargeStats.addBestFit`` (best-fit files) and ``ConvergeStats`` (the .converge file).
"""

import decimal

import numpy as np

from .paramnames import ParamInfo, ParamList

_sci_tolerance = 4  # types.py:13: an exponent is pulled out of a number only when it is larger than this in magnitude


class TextFile:
    """types.py:16-24: lines of text, written joined by newlines"""

    def __init__(self, lines=None):
        self.lines = [lines] if isinstance(lines, str) else (lines or [])

    def write(self, outfile):
        with open(outfile, "w", encoding="utf-8") as f:
            f.write("\n".join(self.lines))


def texEscapeText(string):
    """types.py:27-28: an underscore of plain text as LaTeX prints it"""
    return string.replace("_", "{\\textunderscore}")


def times_ten_power(exponent):
    """types.py:31-32"""
    return "\\cdot 10^{%d}" % exponent


def float_to_decimal(f):
    """types.py:35-46: the Decimal that equals the binary number exactly.  (A double is a dyadic rational, so its decimal
    expansion is finite and Decimal's own conversion of a float already is that expansion.)"""
    if isinstance(f, decimal.Decimal):
        return f
    return decimal.Decimal(float(f))


def _exact(number):
    try:
        return decimal.Decimal(number)  # float, numpy.float64 (a float), int and Decimal: exact
    except TypeError:
        return float_to_decimal(number)


def _scaled(x, exponent):
    """x * 10**-exponent the way the reference forms it (types.py:60,116): the double 10.0**-exponent expanded exactly,
    and the product rounded by the current decimal context (28 digits unless the caller changed it)."""
    return decimal.getcontext().multiply(float_to_decimal(x), float_to_decimal(10.0 ** -exponent))


def numberFigs(number, sigfig, sci=False):
    """types.py:50-92: ``number`` to ``sigfig`` significant figures as positional text.  The digits are those of the
    exact decimal expansion of the double; the figure after the last one kept decides the rounding (5 and above: away
    from zero), and a rounding that carries into a new leading digit (9.996 -> 10.00) moves the decimal point.  With
    ``sci`` the result is (text, exponent): a power of ten is taken out when it is beyond +-4, else the exponent is 0."""
    assert sigfig > 0
    d = _exact(number)
    exponent = 0
    if sci:
        exponent = d.adjusted()
        if abs(exponent) > _sci_tolerance:
            d = _scaled(d, exponent)
        else:
            exponent = 0
    negative, digits = d.as_tuple()[:2]
    lead = d.adjusted()  # power of ten of the first digit
    digits = list(digits) + [0] * (sigfig - len(digits))
    kept = int("".join(str(k) for k in digits[:sigfig]))
    if len(digits) > sigfig and digits[sigfig] >= 5:
        kept += 1
    figs = str(kept)
    lead += len(figs) - sigfig  # one longer after a carry; shorter only for zero, whose figures collapse to "0"
    figs = figs[:sigfig]
    if lead >= sigfig - 1:
        text = figs + "0" * (lead - sigfig + 1)
    elif lead >= 0:
        text = figs[:lead + 1] + "." + figs[lead + 1:]
    else:
        text = "0." + "0" * (-lead - 1) + figs
    if negative:
        text = "-" + text
    return (text, exponent) if sci else text


class NumberFormatter:
    """types.py:95-169: a value and its errors to matching numbers of decimal places"""

    def __init__(self, sig_figs=4, separate_limit_tol=0.1, err_sf=2):
        self.sig_figs = sig_figs
        self.separate_limit_tol = separate_limit_tol
        self.err_sf = err_sf

    def namesigFigs(self, value, limplus, limminus, wantSign=True, sci=False):
        """types.py:102-141: (value, +error, -error[, exponent]) as text.  The figures of the value follow the relative
        size of the upper error; then the value loses figures until it has no more decimal places than the errors, and
        gains them until it has as many as the upper error."""
        frac = limplus / (abs(value) + limplus)
        sf = self.sig_figs
        if frac > 0.1 and 20 <= value < 100:
            sf = 2
        elif frac > 0.01 and value < 1000:
            sf = 3
        err_sf = 1 if (value >= 20 and frac > 0.1 and limplus >= 2) else self.err_sf
        exponent = 0
        if sci:
            # the exponent is that of the larger end of the interval, and all three numbers are scaled by it
            exponent = self.formatNumber(max(abs(value - limminus), abs(value + limplus)), sci=True)[1]
            if exponent:
                value, limplus, limminus = (_scaled(x, exponent) for x in (value, limplus, limminus))
        plus_str = self.formatNumber(limplus, err_sf, wantSign)
        minus_str = self.formatNumber(limminus, err_sf, wantSign)
        res = self.formatNumber(value, sf)
        err_dp = max(self.decimal_places(plus_str), self.decimal_places(minus_str))
        while self.decimal_places(res) > err_dp:
            sf -= 1
            if sf == 0:  # no figure of the value is left at the errors' precision: fixed point, and a plain zero
                fixed = "%." + str(err_dp) + "f"
                res = fixed % value
                if float(res) == 0.0:
                    res = fixed % 0
                break
            res = self.formatNumber(value, sf)
        while self.decimal_places(res) < self.decimal_places(plus_str):
            sf += 1
            res = self.formatNumber(value, sf)
        if sci:
            return res, plus_str, minus_str, exponent
        return res, plus_str, minus_str

    def formatNumber(self, value, sig_figs=None, wantSign=False, sci=False):
        """types.py:144-160: ``wantSign`` puts a + before a positive result (a result that prints as zero gets none)"""
        s = numberFigs(value, self.sig_figs if sig_figs is None else sig_figs, sci=sci)
        exponent = None
        if sci:
            s, exponent = s
        if wantSign and float(s) > 0:
            s = "+" + s
        return (s, exponent) if sci else s

    def decimal_places(self, s):
        """types.py:162-166 (a point in the first position counts as none, as there)"""
        i = s.find(".")
        return len(s) - i - 1 if i > 0 else 0

    def plusMinusLimit(self, limit, upper, lower):
        """types.py:168-169: whether to print the two errors apart: always beyond the first limit, and at the first one
        when they differ by more than the tolerance"""
        return limit != 1 or abs(abs(upper / lower) - 1) > self.separate_limit_tol


class TableFormatter:
    """types.py:172-247: the LaTeX pieces of a boxed table"""

    def __init__(self):
        self.border = "|"
        self.endofrow = "\\\\"
        self.hline = "\\hline"
        self.paramText = "Parameter"
        self.aboveTitles = self.hline
        self.majorDividor = "|"
        self.minorDividor = "|"
        self.colDividor = "||"
        self.belowTitles = ""
        self.headerWrapper = " %s"
        self.noConstraint = "---"
        self.spacer = " "
        self.colSeparator = self.spacer + "&" + self.spacer
        self.numberFormatter = NumberFormatter()

    def getLine(self, position=None):
        """The rule for a named position (``aboveHeader``, ``belowRow``, ...): the attribute of that name where the
        formatter has one, a plain \\hline otherwise."""
        if position is not None and hasattr(self, position):
            return getattr(self, position)
        return self.hline

    def belowTitleLine(self, colsPerParam, numResults=None):
        return self.getLine("belowTitles")

    def startTable(self, ncol, colsPerResult, numResults):
        result_cols = self.majorDividor + (" c" + self.minorDividor) * (colsPerResult - 1) + " c"
        block = " l " + result_cols * numResults
        return "\\begin{tabular} {" + self.border + block + (self.colDividor + block) * (ncol - 1) + self.border + "}"

    def endTable(self):
        return "\\end{tabular}"

    def titleSubColumn(self, colsPerResult, title):
        align = self.majorDividor + "c" + self.majorDividor
        return " \\multicolumn{%d}{%s}{%s}" % (colsPerResult, align, self.formatTitle(title))

    def formatTitle(self, title):
        return "\\bf " + texEscapeText(title)

    def texEquation(self, txt):
        return "$" + txt + "$" if txt and txt[0] != "$" else txt

    def textAsColumn(self, txt, latex=False, separator=False, bold=False):
        """A cell padded to 28 characters, counting the $ signs and the \\boldmath wrapper it is about to get"""
        width = len(txt) + (2 if latex else 0) + (11 if latex and bold else 0)
        res = txt + self.spacer * max(0, 28 - width)
        if latex:
            res = self.texEquation(res)
            if bold:
                res = "{\\boldmath" + res + "}"
        if separator:
            res += self.colSeparator
        return res


class OpenTableFormatter(TableFormatter):
    """types.py:250-264: no outer border, double rule above the titles"""

    def __init__(self):
        super().__init__()
        self.border = ""
        self.aboveTitles = "\\noalign{\\vskip 3pt}" + self.hline + "\\noalign{\\vskip 1.5pt}" + self.hline + "\\noalign{\\vskip 5pt}"
        self.belowTitles = "\\noalign{\\vskip 3pt}" + self.hline
        self.aboveHeader = ""
        self.belowHeader = self.hline
        self.minorDividor = ""
        self.belowFinalRow = ""

    def titleSubColumn(self, colsPerResult, title):
        return " \\multicolumn{%d}{c}{%s}" % (colsPerResult, self.formatTitle(title))


class NoLineTableFormatter(OpenTableFormatter):
    """types.py:267-280: rules only under the header, under a block of parameters and at the end"""

    def __init__(self):
        super().__init__()
        self.aboveHeader = ""
        self.minorDividor = ""
        self.majorDividor = ""
        self.belowFinalRow = self.hline
        self.belowBlockRow = self.hline
        self.colDividor = "|"
        self.hline = ""

    def belowTitleLine(self, colsPerParam, numResults=None):
        return "\\noalign{\\vskip 3pt}\\cline{2-%d}\\noalign{\\vskip 3pt}" % (colsPerParam * numResults + 1)


class ResultTable:
    """
    types.py:283-461: a LaTeX table of parameter constraints.

    ``results``: a MargeStats, a list of them (compared side by side), or objects with a ``getMargeStats`` method (a
    sample set), which is called.  ``limit``: which stored limit to print (1 = the first contour).  ``tableParamNames``
    / ``paramList``: the parameters to list (default: those of the first result).  ``titles``: one per result.
    ``blockEndParams``: in a one-column table, names after which a block rule is drawn.  ``refResults`` with
    ``shiftSigma_indep`` / ``shiftSigma_subset``: print the shift of each mean from a reference result.
    The table is laid out column-major: ``ncol`` parameter columns of ceil(nparams / ncol) rows, the last one padded.
    ``tablePNG`` of the reference is not provided.
    """

    def __init__(self, ncol, results, limit=2, tableParamNames=None, titles=None, formatter=None, numFormatter=None,
                 blockEndParams=None, paramList=None, refResults=None, shiftSigma_indep=False, shiftSigma_subset=False):
        results = list(results) if isinstance(results, (list, tuple)) else [results]
        self.results = [r.getMargeStats() if hasattr(r, "getMargeStats") else r for r in results]
        self.format = NoLineTableFormatter() if formatter is None else formatter
        if numFormatter is not None:
            self.format.numFormatter = numFormatter  # (the attribute the reference sets; numbers use .numberFormatter)
        self.ncol = ncol
        self.tableParamNames = self.results[0] if tableParamNames is None else tableParamNames
        if paramList is not None:
            self.tableParamNames = self.tableParamNames.filteredCopy(paramList)
        self.boldBaseParameters = True
        self.limit = limit
        self.colsPerResult = len(self.results[0].getColumnLabels(limit))
        self.colsPerParam = len(self.results) * self.colsPerResult
        self.refResults = refResults
        self.shiftSigma_indep = shiftSigma_indep
        self.shiftSigma_subset = shiftSigma_subset

        pars = self.tableParamNames.names
        numrow = -(-len(pars) // ncol)
        rows = [pars[r::numrow][:ncol] for r in range(numrow)]
        self.lines = [self.format.startTable(ncol, self.colsPerResult, len(self.results))]
        if titles is not None:
            self.addTitlesRow(titles)
        self.addHeaderRow()
        for r, row in enumerate(rows):
            self.addFullTableRow(row)
            if r == numrow - 1:
                self.addLine("belowFinalRow")
            elif ncol == 1 and blockEndParams is not None and row[0].name in blockEndParams:
                self.addLine("belowBlockRow")
            else:
                self.addLine("belowRow")
        self.endTable()

    def addLine(self, position):
        line = self.format.getLine(position)
        if line is not None:  # a formatter switches a rule off with None
            self.lines.append(line)

    def addTitlesRow(self, titles):
        self.addLine("aboveTitles")
        cols = [self.format.titleSubColumn(1, "")] + [self.format.titleSubColumn(self.colsPerResult, t) for t in titles]
        self.lines.append(self.format.colSeparator.join(cols * self.ncol) + self.format.endofrow)
        below = self.format.belowTitleLine(self.colsPerResult, self.colsPerParam // self.colsPerResult)
        if below:
            self.lines.append(below)

    def addHeaderRow(self):
        self.addLine("aboveHeader")
        heads = [self.format.paramText] + [s for res in self.results for s in res.getColumnLabels(self.limit)]
        cols = [self.format.headerWrapper % s for s in heads]
        self.lines.append(self.format.colSeparator.join(cols * self.ncol) + self.format.endofrow)
        self.addLine("belowHeader")

    def addFullTableRow(self, row):
        txt = self.format.colSeparator.join(self.paramLabelColumn(par) + self.paramResultsTex(par) for par in row)
        # a short last row of a multi-column table: empty cells for the missing parameters
        txt += self.format.colSeparator * ((1 + self.colsPerParam) * (self.ncol - len(row)))
        self.lines.append(txt + self.format.endofrow)

    def paramLabelColumn(self, param):
        return self.format.textAsColumn(param.getLabel(), True, separator=True, bold=not param.isDerived)

    def paramResultsTex(self, param):
        return self.format.colSeparator.join(self.paramResultTex(res, param) for res in self.results)

    def paramResultTex(self, result, p):
        values = result.texValues(self.format, p, self.limit, self.refResults, shiftSigma_indep=self.shiftSigma_indep,
                                  shiftSigma_subset=self.shiftSigma_subset)
        if values is None:  # this result does not have the parameter
            return self.format.textAsColumn("") * len(result.getColumnLabels(self.limit))
        txt = self.format.textAsColumn(values[1], True, separator=True) if len(values) > 1 else ""
        return txt + self.format.textAsColumn(values[0], values[0] != self.format.noConstraint)

    def endTable(self):
        self.lines.append(self.format.endTable())

    def tableTex(self, document=False, latex_preamble=None, packages=("amsmath", "amssymb", "bm")):
        """types.py:431-452: the table as LaTeX; with ``document`` a complete file that can be compiled by itself"""
        if not document:
            return "\n".join(self.lines)
        head = ["\\documentclass{article}", "\\pagestyle{empty}"] + ["\\usepackage{%s}" % p for p in packages]
        head.append("\\renewcommand{\\arraystretch}{1.5}")
        if latex_preamble:
            head.append(latex_preamble)
        return "\n".join(head + ["\\begin{document}"] + self.lines + ["\\end{document}"])

    def write(self, fname, **kwargs):
        """types.py:454-461: tableTex(**kwargs) to a file"""
        TextFile(self.tableTex(**kwargs)).write(fname)


class ParamResults(ParamList):
    """types.py:532-537: results held as attributes of the ParamInfo objects in ``names``"""


def _file_label(par):
    """The label field of a result file.  A parameter made without a label carries its name as label in this package
    (the reference: an empty label); the files show what the reference writes."""
    return par.label if getattr(par, "_label_given", True) or par.label != par.name else ""


class ParamLimit:
    """A marginalised parameter limit (types.py:652-716): lower, upper and which tails are constrained."""

    def __init__(self, minmax, tag="two"):
        self.lower, self.upper = minmax[0], minmax[1]
        self.twotail = tag == "two"
        self.onetail_upper = tag == ">"
        self.onetail_lower = tag == "<"

    def limitTag(self):
        return "two" if self.twotail else (">" if self.onetail_upper else ("<" if self.onetail_lower else "none"))

    def limitType(self):
        """types.py:693-709: the tag in words"""
        return {"two": "two tail", ">": "one tail upper limit", "<": "one tail lower limit", "none": "none"}[self.limitTag()]

    def __str__(self):
        return f"{self.lower:g} {self.upper:g} {self.limitTag()}"


class MargeStats(ParamResults):
    """types.MargeStats (types.py:718-897): per-parameter mean, err and limits per contour (on ``names[i].mean``,
    ``.err``, ``.limits``), their .margestats text (written and read back) and their LaTeX form."""

    def __init__(self, names=None, limits=None):
        super().__init__()
        if names is not None:
            self.names = names
        self.limits = limits
        self.hasBestFit = False

    def loadFromFile(self, filename):
        """types.py:739-764: read a .margestats file.  (A line without a label gives an empty label here; the reference
        takes the last limit tag for it.)"""
        lines = self.fileList(filename)
        self.limits = [float(s.strip()) for s in lines[0].split(":")[1].split(";")]
        self.hasBestFit = False
        nfield = 3 + 3 * len(self.limits)
        for line in lines[3:]:
            if not line.strip():
                break
            items = [s.strip() for s in line.split(None, nfield)]
            name = items[0]
            par = ParamInfo(name.rstrip("*"), items[nfield] if len(items) > nfield else None)
            par.isDerived = name.endswith("*")
            par.mean, par.err = float(items[1]), float(items[2])
            par.limits = [ParamLimit([float(items[k]), float(items[k + 1])], items[k + 2]) for k in range(3, nfield, 3)]
            self.names.append(par)
        return self

    def headerLine(self, inc_limits=False):
        """types.py:766-782: (column header, format of the name column).  ``inc_limits`` names the limit columns by
        their percentage instead of by their number."""
        parForm = self.parFormat()
        text = parForm % "parameter" + "  " + "%-15s%-15s" % ("mean", "sddev")
        for j, limit in enumerate(self.limits):
            tag, last = ("_%.0f%%" % (limit * 100), "type") if inc_limits else (str(j + 1), "limit" + str(j + 1))
            text += "%-15s%-15s%-7s" % ("lower" + tag, "upper" + tag, last)
        return text, parForm

    def __str__(self):
        """types.py:784-798: the .margestats text"""
        header, parForm = self.headerLine()
        text = "Marginalized limits: %s\n\n%s\n" % ("; ".join(str(c) for c in self.limits), header)
        for j, par in enumerate(self.names):
            text += parForm % self.name(j, True) + "%15.7E%15.7E" % (par.mean, par.err)
            for lim in par.limits:
                text += "%15.7E%15.7E  %-5s" % (lim.lower, lim.upper, lim.limitTag())
            text += "   %s\n" % _file_label(par)
        return text

    def limitText(self, limit):
        """types.py:811-815: the percentage of limit number ``limit`` (from 1)"""
        txt = str(round(self.limits[limit - 1] * 100.0))
        return txt.split(".")[0] if txt.endswith(".0") else txt

    def getColumnLabels(self, limit=2):
        """types.py:817-822"""
        return (["Best fit"] if self.hasBestFit else []) + [self.limitText(limit) + "\\% limits"]

    def texValues(self, formatter, p, limit=2, refResults=None, shiftSigma_indep=False, shiftSigma_subset=False):
        """
        types.py:824-897: [LaTeX of the constraint on parameter ``p`` (a name or a ParamInfo)], None if it is not here.

        - a name starting with ``chi2``: mean +- sigma at the first limit, mean and effective degrees of freedom beyond;
        - two tails: mean +- sigma when this is the first limit and the two errors agree within the formatter's
          tolerance, mean^{+upper}_{-lower} otherwise; a common power of ten is taken out of both;
        - one tail: ``< upper`` or ``> lower`` to three figures;
        - neither end constrained: the formatter's ``noConstraint``.
        With ``refResults`` the shift of the mean from that result follows in brackets: in the reference's sigma, or with
        ``shiftSigma_subset`` / ``shiftSigma_indep`` in the sigma of a data subset / of independent data.
        """
        par = self.parWithName(p if isinstance(p, str) else p.name)
        if par is None:
            return None
        nf = formatter.numberFormatter
        lim = par.limits[limit - 1]
        if par.name.startswith("chi2"):
            res, sigma, _ = nf.namesigFigs(par.mean, par.err, par.err, wantSign=False, sci=False)
            res += ("\\pm " + sigma) if limit == 1 else "\\,({\\nu\\rm{:}\\,%.1f})" % (par.err ** 2 / 2)
        elif lim.twotail:
            if nf.plusMinusLimit(limit, lim.upper - par.mean, lim.lower - par.mean):
                res, plus, minus, exponent = nf.namesigFigs(par.mean, lim.upper - par.mean, lim.lower - par.mean, sci=True)
                res += "^{" + plus + "}_{" + minus + "}"
            else:
                res, plus, _, exponent = nf.namesigFigs(par.mean, par.err, par.err, wantSign=False, sci=True)
                res += "\\pm " + plus
            if exponent:
                res = "\\left(\\,%s\\,\\right)" % res + times_ten_power(exponent)
        elif lim.onetail_upper or lim.onetail_lower:
            num, exponent = nf.formatNumber(lim.upper if lim.onetail_upper else lim.lower, 3, sci=True)
            res = ("< " if lim.onetail_upper else "> ") + num + (times_ten_power(exponent) if exponent else "")
        else:
            res = formatter.noConstraint
        ref = refResults.parWithName(par.name) if refResults is not None and res != formatter.noConstraint else None
        if ref is not None:
            delta = par.mean - ref.mean
            if shiftSigma_indep or shiftSigma_subset:
                res += "\\quad("
                if shiftSigma_subset:  # sigma of the difference when one data set contains the other, floored
                    subset_sigma = np.sqrt(abs(par.err ** 2 - ref.err ** 2))
                    res += "%+.1f \\sigma_s" % (delta / max(subset_sigma, ref.err / 20))
                if shiftSigma_indep:
                    res += ", %+.1f \\sigma_i" % (delta / np.sqrt(par.err ** 2 + ref.err ** 2))
                res += ")"
            else:
                res += "\\quad(%+.1f \\sigma)" % (delta / ref.err)
        return [res]


class LikeStats(ParamResults):
    """types.LikeStats (types.py:900-955): posterior statistics of the sample log-likelihoods; the N-D
    confidence-region limits and the best-fit sample live on ``names[i]`` (ND_limit_bot / ND_limit_top / bestfit_sample).
    str() is the .likestats text; loadFromFile reads the scalar summary back (as in the reference, not the table)."""

    def __init__(self):
        super().__init__()
        self.logLike_sample = self.logMeanInvLike = self.meanLogLike = self.logMeanLike = None
        self.complexity = self.varLogLike = None

    def loadFromFile(self, filename):
        """types.py:909-926: the ``name = value`` lines up to the first empty line"""
        found = {}
        for line in self.fileList(filename):
            if not line.strip():
                break
            key, value = (s.strip() for s in line.split("="))
            found[key] = float(value)
        self.logLike_sample = found.get("Best fit sample -log(Like)")
        self.logMeanInvLike = found.get("Ln(mean 1/like)")
        self.meanLogLike = found.get("mean(-Ln(like))")
        self.logMeanLike = found.get("-Ln(mean like)")
        self.complexity = found.get("complexity")
        twice_var = found.get("2*Var(Ln(like))")
        self.varLogLike = None if twice_var is None else 0.5 * twice_var
        return self

    def likeSummary(self):
        text = "Best fit sample -log(Like) = %f\n" % self.logLike_sample
        if self.logMeanInvLike:
            text += "Ln(mean 1/like) = %f\n" % self.logMeanInvLike
        text += "mean(-Ln(like)) = %f\n" % self.meanLogLike
        text += "-Ln(mean like)  = %f\n" % self.logMeanLike
        text += "2*Var(Ln(like)) = %f\n" % (self.varLogLike * 2.0)
        return text

    def headerLine(self):
        """types.py:941-942"""
        return self.parFormat() % "parameter" + "  bestfit        lower1         upper1         lower2         upper2\n"

    def __str__(self):
        """types.py:944-955: the summary, then best-fit sample and the first two N-D limits per parameter"""
        text = self.likeSummary()
        if not self.names:
            return text
        parForm = self.parFormat()
        text += "\n" + self.headerLine()
        for j, par in enumerate(self.names):
            bot, top = np.asarray(par.ND_limit_bot), np.asarray(par.ND_limit_top)
            if bot.size < 2:
                raise Exception("Likestats output assumes at least two contour levels")
            text += parForm % self.name(j, True)
            text += "%15.7E%15.7E%15.7E%15.7E%15.7E" % (par.bestfit_sample, bot[0], top[0], bot[1], top[1])
            text += "   %s\n" % _file_label(par)
        return text
