"""Why does the feature stream idle between RCNN(i-1) and RPN(i+1)?  Logs, per step: the gap on the stream, whether the geometry
event RPN waits for had already completed when the host enqueued the wait, and how far the host is ahead of the GPU."""
import importlib, os, sys, time, collections
import numpy as np, torch
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__))); sys.path.insert(0, ROOT)
PKG = "3d_adapt_auto_driving_amd"
C = importlib.import_module(PKG + ".config"); E = importlib.import_module(PKG + ".eval_rcnn"); S = importlib.import_module(PKG + ".synth")
dev = torch.device("cuda", 0); cfg = C.default_eval_cfg(); model = E.build_model(cfg, dev, seed=0)
batches = [torch.from_numpy(S.scenes(8, 16384, seed0=s * 8)).to(dev) for s in range(6)]
runner = E.PipelinedRunner(model, cfg, dev, **({'depth': int(os.environ['GAP_DEPTH'])} if os.environ.get('GAP_DEPTH') else {}))
eng = runner.engine
log = []
real_rpn, real_rcnn = eng.rpn_stage, eng.rcnn_features
if os.environ.get("GAP_USER_MAIN") == "1":
    torch.cuda.set_stream(torch.cuda.Stream(dev))
main = torch.cuda.current_stream(dev)
real_wait = torch.cuda.Stream.wait_event
waits = []
seen = set()
SKIP = os.environ.get("GAP_SKIP_REPEAT") == "1"
def wait_event(self, ev):
    if self == main:
        waits.append((time.perf_counter(), bool(ev.query())))
        if SKIP and id(ev) in seen:
            return None                      # timing experiment only: the group's event was already waited for by an earlier batch
        seen.add(id(ev))
    return real_wait(self, ev)
torch.cuda.Stream.wait_event = wait_event
def rpn(*a, **k):
    e0 = torch.cuda.Event(enable_timing=True); e1 = torch.cuda.Event(enable_timing=True)
    t = time.perf_counter(); e0.record(main); r = real_rpn(*a, **k); e1.record(main)
    log.append(("rpn", e0, e1, t, list(waits[-2:]))); return r
def rcnn(*a, **k):
    e0 = torch.cuda.Event(enable_timing=True); e1 = torch.cuda.Event(enable_timing=True)
    t = time.perf_counter(); e0.record(main); r = real_rcnn(*a, **k); e1.record(main)
    log.append(("rcnn", e0, e1, t, [])); return r
eng.rpn_stage, eng.rcnn_features = rpn, rcnn
if os.environ.get("GAP_NO_FINAL") == "1":
    importlib.import_module(PKG + ".runners").postprocess = lambda cfg, ret, B: {}
def loop(n):
    for i in range(n):
        runner.submit(batches[i % 6], [batches[(i + d) % 6] for d in range(1, runner.depth + 1)])
    runner.drain()
loop(10); torch.cuda.synchronize(); log.clear()
origin = torch.cuda.Event(enable_timing=True); origin.record(main); t_origin = time.perf_counter()
loop(24); torch.cuda.synchronize()
rows = [(tag, origin.elapsed_time(a0), origin.elapsed_time(a1), (t - t_origin) * 1e3, w) for tag, a0, a1, t, w in log]
prev_end = None
gaps = []
for tag, s, e, th, w in rows[8:48]:
    if tag == "rpn" and prev_end is not None: gaps.append(s - prev_end)
    prev_end = e
print("gaps before RPN (ms):", [round(g, 2) for g in gaps], "mean %.3f" % float(np.mean(gaps)), " period %.3f ms" % ((rows[46][1] - rows[8][1]) / 19))
prev_end = None
for tag, s, e, th, w in rows[8:16]:
    gap = None if prev_end is None else s - prev_end
    print("%-5s gpu %7.2f -> %7.2f  (%.2f ms)  gap before %s   host enqueued at %7.2f ms (lead %.2f ms)  waits %s" % (
        tag, s, e, e - s, "  -  " if gap is None else "%5.2f" % gap, th, s - th, [q for _, q in w]))
    prev_end = e
