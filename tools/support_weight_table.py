"""Host only: what SchedConfig::support_weight does to the schedules of six 1000-gate circuits at n = 30 (the bench circuit and
random_gates seeds 1..5), unplanned and as the planning step's model chooses (qsim_plan_choice).  A pass is priced with the committed
pass-time model, share x (7.16 + 0.43 max(0, blocks - 4)) + 0.03 ms, once on its coordinate share (what choose_schedule ranks by) and
once on the share it runs at, (visited + read_share) / 2 of Circuit.regions().  Usage: support_weight_table.py [n] [--passes]"""
import os, sys
sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), '..'))
from gpu_quantum_simulator_amd import Circuit, circuits

n = int(sys.argv[1]) if len(sys.argv) > 1 and sys.argv[1].isdigit() else 30
show_passes = "--passes" in sys.argv
seeds = [20240117 + n, 1, 2, 3, 4, 5]


def blocks_per_pass(c, setting):
    flips = [] if setting.get("defer") else None
    cnt = {}
    for s in c.schedule(setting=setting, flips=flips):
        if s[1] == "tile" and len(s[3]) > 0:
            cnt[s[0]] = cnt.get(s[0], 0) + 1
    return cnt


def price(c, setting):
    """(model-ms as run, sum of as-run shares, full sweeps, per-pass rows) of the schedule under `setting`."""
    regs = c.regions(setting=setting)
    blocks = blocks_per_pass(c, setting)
    ms = total = 0.0
    full = 0
    rows = []
    for i, r in enumerate(regs):
        share = (r["visited"] + r["read_share"]) / 2
        b = blocks.get(i, 1)
        ms += share * (7.16 + 0.43 * max(0, b - 4)) + 0.03
        total += share
        full += share == 1.0
        rows.append((i, r["kernel"], r["visited"], r["read_share"], b))
    return ms, total, full, rows


def label(h):
    return (f"com {h['commute']} margin {h['cheap_margin']:g} la {h['lookahead']} cap {h['cap']} seed {h['seed']} defer {h['defer']} "
            f"supw {h['support_weight']}")


print(f"n = {n}, 1000 gates; model-ms as run / sum of shares / full sweeps")
tot = {}
for seed in seeds:
    c = Circuit.from_gates(n, circuits.random_gates(n, 1000, seed, "all"))
    line = [f"seed {seed:9d}:"]
    for w in (0, 5, 10):
        ms, shares, full, _ = price(c, {"defer": 1, "support_weight": w})
        tot[w] = tot.get(w, 0.0) + ms
        line.append(f"unplanned w={w}: {ms:5.1f} / {shares:5.2f} / {full}")
    print("   ".join(line), flush=True)
    choice = c.plan_choice()
    cands = choice["candidates"]
    # what the parent's candidate list would have chosen: the same reduction over the candidates without a weight and without the
    # halved margin (their order among themselves is the parent's, except that the parent seeds the best three of the whole list)
    best = {}
    for fam, keep in (("all", lambda h: True), ("w0", lambda h: h["support_weight"] == 0), ("w>0", lambda h: h["support_weight"] > 0)):
        pick = None
        for i, h in enumerate(cands):
            if keep(h) and (pick is None or h["cost_bytes"] < cands[pick]["cost_bytes"] * 0.995):
                pick = i
        best[fam] = pick
    for fam in ("w0", "w>0"):
        h = cands[best[fam]]
        ms, shares, full, rows = price(c, h)
        chosen = " (the model's choice)" if best[fam] == choice["chosen"] else ""
        print(f"    model's best of {fam:3s}: cost {h['cost_bytes'] / (32.0 * 2 ** n):5.2f} sweeps by pass_time_cost; as run {ms:5.1f} ms / {shares:5.2f} / {full}"
              f"   [{label(h)}]{chosen}")
        if show_passes:
            for i, kern, vis, rd, b in rows:
                print(f"        pass {i:2d} {kern:5s} visited {vis:.5f} read {rd:.5f} blocks {b}")
    # ... and whether the coordinate ranking sees the schedules that run cheapest: the five cheapest as run among the model's best 24
    order = sorted(range(len(cands)), key=lambda i: cands[i]["cost_bytes"])[:24]
    seen = sorted(((price(c, cands[i])[0], rank, i) for rank, i in enumerate(order)))[:5]
    print("    cheapest as run among the model's best 24 (as-run ms, model rank, weight): " +
          ", ".join(f"{ms:.1f} #{rank} w{cands[i]['support_weight']}" for ms, rank, i in seen))
    print(f"    {len(cands)} candidates ranked in {choice['seconds']:.2f} s", flush=True)
print("unplanned totals: " + ", ".join(f"w={w}: {v:.1f}" for w, v in tot.items()))
