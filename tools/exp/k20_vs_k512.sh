set -u
export TMPDIR=/tmp
K=$(mktemp)
for r in 1 2 3; do
  python bench.py --full --steps 20 --warmup 5 --no-cpu --headline-only --repeats 9 > $K 2>/dev/null
  python3 -c "
import json, sys; d=json.load(open(sys.argv[1])); t=d['config']['timed_region']; print('K=20  median %.3f  windows %s  strict %.0f rates %s' % (d['ms_per_step']*1e3, t['windows_us_per_step'], d['roofline']['strict_bracket_ns_per_step'], t['us_per_step_by_stream_rates']))" $K
  python bench.py --full --steps 512 --warmup 64 --no-cpu --headline-only > $K 2>/dev/null
  python3 -c "
import json, sys; d=json.load(open(sys.argv[1])); t=d['config']['timed_region']; print('K=512 median %.3f  windows %s' % (d['ms_per_step']*1e3, t['windows_us_per_step']))" $K
done
rm -f $K
