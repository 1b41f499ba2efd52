# on the GPU box: full GPU suite + one bench line (isolated kernel times)
timeout 400 python -m pytest tests -q -m gpu --timeout=300 -x 2>&1 | tail -3
python bench.py --full 2>/dev/null | tail -1 | python -c "
import json,sys
d=json.loads(sys.stdin.read()); print(d['value'], d['ms_per_step'], d['matches_last_frame']); print(d['roofline']['isolated']['kernel_ms_per_step'])"
