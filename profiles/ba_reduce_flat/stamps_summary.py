"""summary of the stamps of d_reduce2: python stamps_summary.py DIR  (DIR holds stamps_legacy.npz and stamps_flat.npz: `stamps` =
[runs][workgroup][8] 100 MHz ticks, 0 = slot not stamped; `P`; `flat_slots`).  Dated record: it produced stamps_summary.txt."""
import numpy as np, sys
for name in ("legacy","flat"):
    z=np.load(f"{sys.argv[1]}/stamps_{name}.npz")
    S=z["stamps"]; P=int(z["P"]); ndiag=(P+1+7)&~7
    print("==",name,"runs",S.shape[0],"flat_slots",int(z["flat_slots"]))
    for run in range(S.shape[0]):
        st=S[run].astype(np.int64)
        valid=(st[:,0]>0)&(st[:,7]>0)
        t0=st[valid,0].min()
        rel=(st-t0)*0.01  # us (100 MHz)
        diag=np.zeros(4096,bool); diag[:P]=True; diag&=valid
        off=np.zeros(4096,bool); off[ndiag:]=True; off&=valid
        end=rel[valid,7].max()
        print(f"run {run}: valid {valid.sum()} diag {diag.sum()} off {off.sum()}  kernel span (first start -> last end) {end:.2f} us; last end: diag {rel[diag,7].max():.2f} off {rel[off,7].max():.2f}; starts: diag max {rel[diag,0].max():.2f} off max {rel[off,0].max():.2f}")
        # off-diagonal links (thread 0 of the wg)
        o=rel[off]
        seg=[("start->record/grp",0,1),("->indices/blk",1,2),("->(odo before loop)",2,3),("->W round 1",3,4),("->all rounds",4,5),("->barrier",5,6),("->end(odo+store)",6,7)]
        def q(x): return "med %.2f p90 %.2f max %.2f"%(np.median(x),np.percentile(x,90),x.max())
        for nm,a,b in seg:
            ok=(o[:,a]>-1e5)&(o[:,b]>-1e5)&(st[off][:,a]>0)&(st[off][:,b]>0)
            print("   off %-22s %s  (n=%d)"%(nm,q(o[ok,b]-o[ok,a]),ok.sum()))
        print("   off total                 ",q(o[:,7]-o[:,0]))
        # slowest 5% of off wgs by end time: their link breakdown
        idx=np.argsort(o[:,7])[-max(10,len(o)//20):]
        print("   off LAST 5%% to end: start med %.2f; tail seg (barrier->end) med %.2f max %.2f; total med %.2f"%(np.median(o[idx,0]),np.median(o[idx,7]-o[idx,6]),(o[idx,7]-o[idx,6]).max(),np.median(o[idx,7]-o[idx,0])))
        long_tail=(o[:,7]-o[:,6])>0.8
        print("   off wgs with barrier->end > 0.8us: %d, their end med %.2f max %.2f ; others end med %.2f max %.2f"%(long_tail.sum(), np.median(o[long_tail,7]) if long_tail.any() else -1, o[long_tail,7].max() if long_tail.any() else -1, np.median(o[~long_tail,7]), o[~long_tail,7].max()))
        dg=rel[diag]; sd=st[diag]
        ok1=(sd[:,1]>0)&(sd[:,2]>0)   # (the fixed pose gathers nothing and stamps no index round)
        print("   diag start->idx %s (n=%d)"%(q(dg[ok1,1]-dg[ok1,0]),ok1.sum()))
        print("   diag idx->Dg gathered %s (n=%d)"%(q(dg[ok1,2]-dg[ok1,1]),ok1.sum()))
        ok=sd[:,3]>0
        print("   diag start->odo lanes done %s (n=%d)"%(q(dg[ok,3]-dg[ok,0]),ok.sum()))
        print("   diag start->gather done %s"%q(dg[:,2]-dg[:,0]))
        print("   diag gather->barrier %s ; barrier->end %s ; total %s"%(q(dg[:,6]-dg[:,2]),q(dg[:,7]-dg[:,6]),q(dg[:,7]-dg[:,0])))
