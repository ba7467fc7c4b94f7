"""The odometry record in the device-resident closed loop (ingvio_odom_begin / _end): OdomForm wraps any Form of
closed_loop.DeviceLoop and takes one record per frame entry without a host synchronisation.

  plain and in-frame forms   odom_begin in ran(i): behind run(i), in front of stage(i + 1), whose IMU steps advance the table's pose
  late forms                 odom_begin at the end of after(i): behind the inner form's own run, so the record carries the GNSS update's
                             or the tail's boxPlus and drop
  odom_end                   in collect(i).  A loop that does not collect (collect=False, the bench tool) ends record i right in front
                             of odom_begin(i + 1) instead - one slot is pending at a time - i.e. behind run(i + 1): the host then waits
                             for nothing that frame i + 1 has to produce.
"""
from ingvio_amd import capi
from ingvio_amd.closed_loop import Form


class OdomForm(Form):
    """dicts=False: the records stay one numpy array of capi.ODOM_DTYPE in a buffer the form reuses (what a compiled host would hold);
    the default hands out a list of dicts per frame, which costs this harness' Python milliseconds for hundreds of filters"""

    def __init__(self, inner=None, what=capi.ODOM_ALL, dicts=True):
        self.inner, self.what, self.dicts = inner or Form(), what, dicts
        self.raw = None
        self.late = self.inner.late
        self.pending = False
        self.last = None                                                 # the records ended last

    def end(self, ctx):
        if self.pending:
            if not self.dicts and self.raw is None:
                self.raw = (capi.Odom * ctx.batch)()
            self.last = ctx.odom_end(self.raw, self.dicts)
            self.pending = False
        return self.last

    def begin(self, ctx):
        self.end(ctx)                                                    # not collected: the slot is freed here
        ctx.odom_begin(0, None, self.what)
        self.pending = True

    def prepare(self, ctx, cases, f):
        return self.inner.prepare(ctx, cases, f)

    def staged(self, loop, i):
        self.inner.staged(loop, i)

    def ran(self, loop, i):
        self.inner.ran(loop, i)
        if not self.late:
            self.begin(loop.ctx)

    def after(self, loop, i):
        self.inner.after(loop, i)
        if self.late:
            self.begin(loop.ctx)

    def collect(self, ctx):
        """-> the frame's records (a list of dicts, one per filter); with an inner form that collects: (its results, the records)"""
        res = self.inner.collect(ctx)
        rec = self.end(ctx)
        return rec if res is None else (res, rec)

    def finish(self, ctx):
        """a loop that did not collect: ends the record still pending"""
        return self.end(ctx)
