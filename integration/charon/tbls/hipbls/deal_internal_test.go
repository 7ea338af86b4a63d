//go:build hipbls

package hipbls

import (
	"testing"

	promtest "github.com/prometheus/client_golang/prometheus/testutil"
	"github.com/stretchr/testify/require"

	"github.com/obolnetwork/charon/tbls"
)

// TestBatchThresholdSplitEqualsSerial: every validator dealt in one call gives what the serial calls of
// dkg/keycast.go give on tbls.Herumi{} for the same shares: the root key, each pubshare, and the secret back from any
// threshold shares; a secret that does not deserialize fails alone; the metrics advance under "threshold_split".
func TestBatchThresholdSplitEqualsSerial(t *testing.T) {
	h, err := New()
	require.NoError(t, err)
	ref := tbls.Herumi{}
	const n, total, threshold = 9, 5, 3
	secrets := make([]tbls.PrivateKey, n)
	for i := range secrets {
		secrets[i], err = ref.GenerateSecretKey()
		require.NoError(t, err)
	}
	for i := range secrets[4] {
		secrets[4][i] = 0xff // above r
	}

	items := func(path string) float64 { return promtest.ToFloat64(itemsCounter.WithLabelValues(path)) }
	failed := func(path string) float64 { return promtest.ToFloat64(failedCounter.WithLabelValues(path)) }
	i0, f0 := items("threshold_split"), failed("threshold_split")
	dealt, errs, err := h.BatchThresholdSplit(secrets, total, threshold)
	require.NoError(t, err)
	require.Len(t, dealt, n)
	require.InDelta(t, n, items("threshold_split")-i0, 0)
	require.InDelta(t, 1, failed("threshold_split")-f0, 0)

	for v, d := range dealt {
		if v == 4 {
			require.ErrorContains(t, errs[v], "cannot unmarshal bytes into Herumi secret key")
			_, serialErr := ref.ThresholdSplit(secrets[v], total, threshold)
			require.Error(t, serialErr)

			continue
		}
		require.NoError(t, errs[v])
		pk, err := ref.SecretToPublicKey(secrets[v])
		require.NoError(t, err)
		require.Equal(t, pk, d.PubKey)
		require.Len(t, d.Shares, total)
		require.Len(t, d.PubShares, total)
		for idx, share := range d.Shares {
			pub, err := ref.SecretToPublicKey(share)
			require.NoError(t, err)
			require.Equal(t, pub, d.PubShares[idx])
		}
		back, err := ref.RecoverSecret(map[int]tbls.PrivateKey{2: d.Shares[2], 4: d.Shares[4], 5: d.Shares[5]}, total, threshold)
		require.NoError(t, err)
		require.Equal(t, secrets[v], back)
	}

	// the serial method is one validator of the same call
	one, err := h.ThresholdSplit(secrets[0], total, threshold)
	require.NoError(t, err)
	back, err := ref.RecoverSecret(map[int]tbls.PrivateKey{1: one[1], 2: one[2], 3: one[3]}, total, threshold)
	require.NoError(t, err)
	require.Equal(t, secrets[0], back)

	none, errs, err := h.BatchThresholdSplit(nil, total, threshold)
	require.NoError(t, err)
	require.Nil(t, none)
	require.Nil(t, errs)
}

// TestBatchRecoverSecretEqualsSerial: every group recovered in one call gives tbls.Herumi{}'s RecoverSecret and
// SecretToPublicKey for that group, error presence included (an empty group, a share above r).
func TestBatchRecoverSecretEqualsSerial(t *testing.T) {
	h, err := New()
	require.NoError(t, err)
	ref := tbls.Herumi{}
	const total, threshold = 5, 3
	var groups []map[int]tbls.PrivateKey
	for g := 0; g < 6; g++ {
		secret, err := ref.GenerateSecretKey()
		require.NoError(t, err)
		shares, err := ref.ThresholdSplit(secret, total, threshold)
		require.NoError(t, err)
		groups = append(groups, map[int]tbls.PrivateKey{1 + g%3: shares[1+g%3], 4: shares[4], 5: shares[5]})
	}
	groups = append(groups, map[int]tbls.PrivateKey{}) // empty
	var big tbls.PrivateKey
	for i := range big {
		big[i] = 0xff
	}
	groups = append(groups, map[int]tbls.PrivateKey{1: groups[0][4], 2: big}) // a share above r

	items := func(path string) float64 { return promtest.ToFloat64(itemsCounter.WithLabelValues(path)) }
	failed := func(path string) float64 { return promtest.ToFloat64(failedCounter.WithLabelValues(path)) }
	i0, f0 := items("recover_secret"), failed("recover_secret")
	secrets, pks, errs, err := h.BatchRecoverSecret(groups)
	require.NoError(t, err)
	require.InDelta(t, len(groups), items("recover_secret")-i0, 0)
	require.InDelta(t, 2, failed("recover_secret")-f0, 0)

	for g, grp := range groups {
		want, serialErr := ref.RecoverSecret(grp, total, threshold)
		if serialErr != nil {
			require.Error(t, errs[g])
			_, oneErr := h.RecoverSecret(grp, total, threshold)
			require.Error(t, oneErr)

			continue
		}
		require.NoError(t, errs[g])
		require.Equal(t, want, secrets[g])
		pk, err := ref.SecretToPublicKey(want)
		require.NoError(t, err)
		require.Equal(t, pk, pks[g])
		one, err := h.RecoverSecret(grp, total, threshold)
		require.NoError(t, err)
		require.Equal(t, want, one)
	}
}
