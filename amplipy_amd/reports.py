"""The host life of an opt-in report of the command line: one class per report, next to its ``Tables`` in
the report's own module, one method per stage of ``amplipy.run_amplipy``, which walks ``REGISTRY`` stage by stage the way
``amplihip.hip`` walks its table of ``HookOps``."""
from __future__ import annotations

from . import qc
from .readloop import print_log


class Report:
    """The defaults of every stage, in the order the run reaches them; a report writes the stages it has.  ``run`` is the one
    object ``run_amplipy`` makes of its keyword arguments (unchanged, under their names) plus dist, rank, world, device, G,
    ref_id, ref_seq, v_min_depth and v_min_freq, with min_quality resolved.  An instance lives for one run and keeps what it
    loaded, opened and collected.

    EVERY RANK MUST ISSUE THE SAME SEQUENCE OF COLLECTIVES.  ``run_amplipy`` calls ``collect`` of the active reports in registry
    order on every rank, so that holds as long as ``active`` depends on the run's arguments alone -- never on the rank or on what
    the rank loaded or read -- and ``collect`` issues its collectives whatever the rank's tables hold."""

    name = None                       # the keyword of calling.vcf_line and VcfWriter: calling.INFO_ORDER has them in registry order
    HEADER_LINES = ""                 # the module's ##INFO lines
    outputs = ()                      # per output file, in the order they are written: (the argument of the run that names it, what
                                      # the log calls it, writer(f, ref_id, tables))
    with_calls = False                # write() runs beside the VCF, in front of the consensus, not behind it
    opened = ()                       # (file, its entry of ``outputs``) of the files rank 0 opened
    tables = None                     # the module's Tables on rank 0 behind collect()
    lost = 0                          # reads a keyed device table had no slot for, on every rank behind collect()

    def active(self, run):
        """Is the report on?"""
        return False

    def check(self, run):
        """The argument errors (readloop.error).  Called whether the report is on or not: an argument that needs the report is one."""

    def load(self, run):
        """Load the input files, with their "Loading ..." log lines (every rank)."""

    def open(self, run):
        """Load the inputs on every rank; open the outputs that are asked for (qc.open_new) on rank 0 only."""
        self.load(run)
        self.opened = []
        for out in self.outputs if run.rank == 0 else ():
            if getattr(run, out[0]) is not None:
                self.opened.append((qc.open_new(getattr(run, out[0])), out))

    def enable(self, run, eng):
        """Switch the engine's hook on."""

    def collect(self, run, eng):
        """Behind the count table's all-reduce: read the engine out, sum over the ranks, make ``tables`` on rank 0."""

    def annotates(self, run):
        """Does an active report put keys on the VCF (the header is written before there are tables)?"""
        return True

    def vcf_tables(self, run):
        """The Tables the VCF records are annotated with, or None."""
        return self.tables if self.annotates(run) else None

    def writer_args(self, arg, run, res):
        """What the writer of the output that ``arg`` names takes behind the file; res: the calling.CallResult."""
        return run.ref_id, self.tables

    def write(self, run, res):
        """The output files and their "Output ..." log lines."""
        for f, (arg, what, writer) in self.opened:
            writer(f, *self.writer_args(arg, run, res))
            print_log("Output %s: %s" % (what, getattr(run, arg)))

    def add_to_qc(self, report):
        """What the QC report's JSON takes from this report."""

    def summary(self, run):
        """The closing log line, where the report's Tables has one."""
        line = getattr(self.tables, "summary_line", None)
        if line is not None:
            print_log(line())

    def after(self, run):
        """Behind the run's last collective: what may end the run with an error."""

    def files(self):
        """The open output files, for the run to close."""
        return [f for f, _ in self.opened]


def __getattr__(name):
    # REGISTRY is made on first use, not on import: every report module imports this one for the base class
    if name != "REGISTRY":
        raise AttributeError(name)
    from . import amplicon, codon, cooc, deletion, errprof, haplotype, readpos, strand
    global REGISTRY
    REGISTRY = (strand.StrandReport, amplicon.AmpliconReport, codon.CodonReport, deletion.DeletionReport, cooc.CoocReport,
                errprof.ErrprofReport, haplotype.HapReport, readpos.ReadposReport)      # HOOK_STRAND .. HOOK_READPOS of amp_hook.hpp (HOOK_INSEV aside: DeletionReport drives it)
    return REGISTRY
