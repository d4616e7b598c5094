"""Summarise the phase stamps of an AZ_TOWER_TRACE build (tools/tower_trace.c): shader-clock cycles
per phase of tower32w_board, mean over the traced workgroups' waves and the 2B residual convs.
Slots per wave: 0 start, 1 planes staged, 2 input conv done, conv i at 3 + 32 i: +0 start, +1 chunk-0
transform barrier, +2+c after chunk c's barrier, +10 core done (before the epilogue), +11 epilogue
written, +12+c before chunk c's barrier, +20+c after step 4 of chunk c, +28+c (c < 4, waves 0-3 of the
256-filter row-direct forms) start of the tail transform of chunk c + 1; 3 + 64 B: heads done.
The two-board kernel (AZ_WINO_BOARDS=2, tower32w_boards2) stamps the same slots for its pair of boards: 1 after
the first board's planes are staged, 2 after both input convs and the copies to global ACT, the conv slots as
above; it has no tail transform (no +28+c).  Pass boards = 2 so that the totals are labelled per pair.
Usage: python tools/tower_trace.py trace.bin [blocks] [boards]"""
import sys

import numpy as np

B = int(sys.argv[2]) if len(sys.argv) > 2 else 20
NB = int(sys.argv[3]) if len(sys.argv) > 3 else 1
UNIT = "pair of boards" if NB == 2 else "board"
NS = 2048
t = np.fromfile(sys.argv[1], np.uint64).astype(np.int64).reshape(8, 8, NS)
wgok = (t[:, :, 0] > 0).all(1)
t = t[wgok]                                           # [wg, waves, NS]
print("traced workgroups: %d" % t.shape[0])
conv = np.stack([t[:, :, 3 + 32 * i: 35 + 32 * i] for i in range(2 * B)], 2)   # [wg, waves, convs, 32]
end = 3 + 64 * 20
total = t[:, :, end] - t[:, :, 0]
print("total %.0f cycles per %s; staging %.0f, input conv%s %.0f, heads %.0f"
      % (total.mean(), UNIT, (t[:, :, 1] - t[:, :, 0]).mean(), " (both boards, second staging, copies to global ACT)" if NB == 2 else "",
         (t[:, :, 2] - t[:, :, 1]).mean(),
         (t[:, :, end] - conv[:, :, -1, 11]).mean()))
per = conv[:, :, :, 11] - conv[:, :, :, 0]
print("conv (start -> epilogue written): mean %.0f  min %.0f  max %.0f" % (per.mean(), per.min(), per.max()))
print("between convs (epilogue barrier + residual reads): mean %.0f" % (conv[:, :, 1:, 0] - conv[:, :, :-1, 11]).mean())
print("xres + chunk-0 transform + barrier: %.0f" % (conv[..., 1] - conv[..., 0]).mean())
print("output transform + resid + relu + store: %.0f" % (conv[..., 11] - conv[..., 10]).mean())
late = np.arange(8) >= 4
for c in range(8):
    start = conv[..., 1 + c]                          # after the barrier that opens chunk c
    s4 = conv[..., 20 + c]
    pre = conv[..., 12 + c]
    post = conv[..., 2 + c]
    print("chunk %d: steps 0-4 %5.0f (early %5.0f late %5.0f)  steps 5-end %6.0f (early %6.0f late %6.0f)  barrier wait %4.0f (early %4.0f late %4.0f)"
          % (c, (s4 - start).mean(), (s4 - start)[:, ~late].mean(), (s4 - start)[:, late].mean(),
             (pre - s4).mean(), (pre - s4)[:, ~late].mean(), (pre - s4)[:, late].mean(),
             (post - pre).mean(), (post - pre)[:, ~late].mean(), (post - pre)[:, late].mean()))
cyc = (conv[..., 9] - conv[..., 1]).mean() / 8
print("mean chunk (barrier to barrier) %.0f cycles per %s; MFMA issue per SIMD and chunk: f32 products 16384 (2 waves x 256 x 32), split-f16 row-direct 4608 per board (2 waves x 144 x 16)" % (cyc, UNIT))
sk = conv.max(1) - conv.min(1)
print("wave skew within a workgroup (max - min), mean: start %.0f, after chunk barriers %.0f, before chunk barriers %.0f, after step 4 %.0f"
      % (sk[..., 0].mean(), sk[..., 2:10].mean(), sk[..., 12:20].mean(), sk[..., 20:28].mean()))
# the tail transform, the barrier waits of the two halves and the conv boundary (256-filter row-direct forms)
early, latew = conv[:, :4], conv[:, 4:]
if (early[..., 28:32] > 0).all():
    tail = early[..., 12:16] - early[..., 28:32]
    print("tail transform, waves 0-3, chunks 0-3: mean %.0f  min %.0f  max %.0f cycles" % (tail.mean(), tail.min(), tail.max()))
    lead = latew[..., 12:16].max(1, keepdims=True) - early[..., 28:32]
    print("last late wave's arrival at the barrier minus tail start: mean %.0f" % lead.mean())
else:
    print("no tail stamps (transform inside the steps, or another form)")
for name, x in (("waves 0-3", early), ("waves 4-7", latew)):
    print("barrier wait %s (chunks 0-6): mean %.0f" % (name, (x[..., 2:9] - x[..., 12:19]).mean()))
arr = conv[..., 12:19]                                # arrival at the chunk barrier [wg, wave, conv, 7]
print("last arrival at the chunk barrier is a wave 0-3 in %.0f %% of chunks" % (100.0 * (arr == arr.max(1, keepdims=True))[:, :4].any(1).mean()))
print("slack of the other half at the barrier: waves 0-3 arrive %.0f cycles after the last of waves 4-7 (negative: before)"
      % (arr[:, :4].max(1) - arr[:, 4:].max(1)).mean())
bd = conv[:, :, 1:, 1] - conv[:, :, :-1, 19]
print("conv boundary (chunk 7 done -> next conv's chunk loop): mean %.0f, waves 0-3 %.0f, waves 4-7 %.0f"
      % (bd.mean(), bd[:, :4].mean(), bd[:, 4:].mean()))
