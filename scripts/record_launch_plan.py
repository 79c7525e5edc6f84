"""Records which launch and which variant runs every op of the model programs, and what they compute (needs the GPU):

    python scripts/record_launch_plan.py [OUT.json]          # default tests/golden/launch_plan.json

For every case of tests/launch_plan_cases.py -- (model, engine max_batch, batch, switches) -- one forward on a seeded input; written per case:
the dd_net_op_launches and dd_net_op_variants vectors and the sha256 of the output tensor (of the decoded arrays in the SSD / YOLO decode
modes).  tests/test_gpu_launch_plan.py holds the executor to the file.  Record it at the commit BEFORE a change to the executor's host code,
twice, and compare the two files: a digest that does not repeat is to be left out of the fixture (--drop-digest ID), its vectors stay."""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))


def main(argv):
    import launch_plan_cases as C
    drop = [argv[i + 1] for i, a in enumerate(argv) if a == '--drop-digest']
    pos = [a for i, a in enumerate(argv) if not a.startswith('--') and (i == 0 or argv[i - 1] != '--drop-digest')]
    out = pos[0] if pos else os.path.join(ROOT, 'tests', 'golden', 'launch_plan.json')
    plan = {}
    for case in C.cases():
        cid = C.case_id(case)
        got = C.run(case)
        if cid in drop:
            got.pop('output', None); got.pop('decoded', None)
        plan[cid] = got
        print(cid, got.get('output', got.get('decoded', '-'))[:16], flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
    with open(out, 'w') as f:
        f.write('{\n' + ',\n'.join('%s: %s' % (json.dumps(k), json.dumps(v, separators=(',', ':'))) for k, v in plan.items()) + '\n}\n')
    print('%d cases -> %s' % (len(plan), out))


if __name__ == '__main__':
    main(sys.argv[1:])
