#!/usr/bin/env python3
"""tools/codegen_compare.py <dir of tree A> <dir of tree B> - env_kernel instantiations of k_physics.hip in two trees, function by function: the
instruction streams (comments dropped, local labels renumbered) and the compiler's resource remarks.  Each directory holds `k_physics.s` and
`remarks.txt` of one tree:

    hipcc --offload-arch=gfx950 -O3 -std=c++17 -fPIC -ffp-contract=off -I<tree>/minppo_amd/csrc -I<tree>/include -Rpass-analysis=kernel-resource-usage \\
          --cuda-device-only -S <tree>/minppo_amd/csrc/k_physics.hip -o <dir>/k_physics.s 2> <dir>/remarks.txt

(cross-compiles: no GPU needed).  Tree A's specialised kernels carry 16 template arguments, tree B's 17 (the number of ball joints in front of cparam):
an instantiation of A is matched with the one of B that has a 0 there.  profiles/ball_joints_codegen.txt is its output."""
import re, sys, hashlib, subprocess
def funcs(path):
    out={}; cur=None; body=[]
    for line in open(path):
        m=re.match(r'^(_ZN4mppo10env_kernelI\S+):\s', line)
        if m: cur=m.group(1); body=[]; continue
        if cur is not None:
            if line.startswith('.Lfunc_end'):
                out[cur]=body; cur=None; continue
            t=line.split(';')[0].rstrip()
            if not t.strip(): continue
            t=re.sub(r'\.LBB\d+_','.LBB_',t)
            t=re.sub(r'\.Lpost_getpc\d+','.Lpost_getpc',t)
            t=re.sub(r'_ZN4mppo\S+','SYM',t)
            body.append(t)
    return out
def remarks(path):
    out={}; cur=None
    for line in open(path):
        m=re.search(r'remark: (.*?) \[-Rpass',line)
        if not m: continue
        t=m.group(1).strip()
        if t.startswith('Function Name:'): cur=t.split(':',1)[1].strip(); out[cur]={}
        elif cur and ':' in t: k,v=t.split(':',1); out[cur][k.strip()]=v.strip()
    return out
def dims(name):
    m=re.search(r'StaticModelI((?:Li\d+E)+)EELi(\d)E',name)
    if not m: return None
    return tuple(int(x) for x in re.findall(r'Li(\d+)E',m.group(1))), int(m.group(2))
old,new=funcs(sys.argv[1]+'/k_physics.s'),funcs(sys.argv[2]+'/k_physics.s')
ro,rn=remarks(sys.argv[1]+'/remarks.txt'),remarks(sys.argv[2]+'/remarks.txt')
keys=('VGPRs','AGPRs','TotalSGPRs','ScratchSize [bytes/lane]','LDS Size [bytes/block]','Occupancy [waves/SIMD]','VGPRs Spill','SGPRs Spill')
short=lambda r:' '.join(f"{k.split(' [')[0].replace(' ','')}={r.get(k,'?')}" for k in keys)
newby={}
for n in new:
    d=dims(n)
    if d: newby[d]=n
print("# env_kernel instantiations of k_physics.hip, parent commit against this tree: hipcc --offload-arch=gfx950 -O3 -std=c++17 -ffp-contract=off")
print("# --cuda-device-only -S -Rpass-analysis=kernel-resource-usage; instruction streams compared line by line after dropping comments and")
print("# renumbering local labels (a specialised kernel's name gains one template argument, the number of ball joints, in front of cparam).")
same=0; tot=0
for n in sorted(old):
    d=dims(n)
    if d is None:
        nn=[x for x in new if x==n]
        nn=nn[0] if nn else None
        mm=re.search(r'RuntimeModelELi(\d)E',n)
        label="RuntimeModel mode "+(mm.group(1) if mm else '?')
    else:
        nd=(d[0][:15]+(0,)+d[0][15:], d[1]); nn=newby.get(nd); label=f"StaticModel{d[0]} mode {d[1]}"
    if nn is None: print(label,"MISSING in the new tree"); continue
    eq = old[n]==new[nn]
    if d is not None: tot+=1; same+=eq
    print(f"{label}\n   parent: {len(old[n])} instructions/directives  {short(ro.get(n,{}))}\n   new   : {len(new[nn])} instructions/directives  {short(rn.get(nn,{}))}\n   instruction streams {'IDENTICAL' if eq else 'DIFFER'}")
for d,n in sorted(newby.items()):
    if d[0][15]!=0:
        print(f"StaticModel{d[0]} mode {d[1]} (new: the ball humanoid)\n   new   : {len(new[n])} instructions/directives  {short(rn.get(n,{}))}")
for n in sorted(new):
    if 'RuntimeBallModel' in n:
        print(f"RuntimeBallModel mode {re.search(r'RuntimeBallModelELi([0-9])E', n).group(1)} (new: the run-time-sized kernel of robots with ball joints)\n   new   : {len(new[n])} instructions/directives  {short(rn.get(n,{}))}")
print(f"# specialised instantiations present in both trees: {same} of {tot} identical")
print("# scratch bytes per lane, every env_kernel of the new tree:", sorted({rn[n].get('ScratchSize [bytes/lane]') for n in rn if 'env_kernel' in n}))
